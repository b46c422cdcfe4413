// hk_host_step.cpp -- hk_step_host behind its argument checks: the pinned buffer, the one bounded wait loop, the
// resident step server's state machine and the three step paths (server, launch per step, staged copies).
#include "hk_host_step.h"

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <string>

namespace hk {
namespace {

using Clock = std::chrono::steady_clock;

// the server's own limits (hk_kernels.h HostServer): it exits after kSrvIdleMs without a request or kSrvLifeMs in
// all; the host replaces it before either can fire mid-request (half those times), and relaunches on demand.  The
// idle limit bounds what a resident server can cost other work: a kernel that lands on the server stream's hardware
// queue (streams share the box's 4 queues) or a device-wide synchronise waits for its idle exit.
constexpr int kSrvIdleMs = 4, kSrvLifeMs = 2000;
// the longest a server-path hk_step_host call waits for its answer, and a stop for the server's stream (the server
// is ordered after the caller's stream, so this also bounds the work queued there before the step); then the call
// fails with HK_E_DEVICE.  HK_STEP_HOST_WAIT_MS (read at a context's first step) replaces it.
constexpr int kSrvWaitMs = 10000;

// At most ONE resident step server per device and process: every single-arena context's server runs on
// the device's one server stream, and a context that starts its server first stops the running one of another
// context.  So N facades stepped round-robin cost a server hand-over per step (a quit, a stream wait and a launch:
// tens of microseconds), never a kernel queued behind another context's idle server.  ``mu`` is held for a whole
// server-path hk_step_host call and by every stop, so a hand-over never interrupts a request in flight on another
// thread.  ``stream`` is created on demand: an abandoned server keeps the one it was launched on.
struct SrvSlot {
  std::mutex mu;
  hipStream_t stream = nullptr;
  StepServer *owner = nullptr;
};
SrvSlot &srv_slot(int device) {
  static SrvSlot slots[kMaxDevices];
  return slots[device];
}

// The one wait loop: spin until *word == seq (word may be null: wait for the stream alone), asking `st` every 4096
// polls, so work that faulted returns its error and work that ended without writing the word is noticed.
enum class Wait { Answered, Idle, Error, Deadline };
Wait wait_word(const volatile uint64_t *word, uint64_t seq, hipStream_t st, const Clock::time_point *deadline,
               hipError_t *err) {
  for (uint32_t k = 1;; ++k) {
    if (word && *word == seq) return Wait::Answered;
    if (word && (k & 4095u) != 0u) continue;
    *err = hipStreamQuery(st);
    if (*err == hipErrorNotReady) {
      if (deadline && Clock::now() >= *deadline) return Wait::Deadline;
      continue;
    }
    if (*err != hipSuccess) return Wait::Error;
    return word && *word == seq ? Wait::Answered : Wait::Idle;
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ HostBuf
hipError_t HostBuf::alloc(bool staged) {
  hipError_t e = hipSuccess;
  if (staged && (e = hipMalloc(&dev, kInBytes + HK_HOST_RECORD_BYTES)) != hipSuccess) return e;
  if ((e = hipHostMalloc(&pin, kBytes, hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess ||
      (e = hipHostGetDevicePointer((void **)&map, pin, 0)) != hipSuccess) {
    release();
    return e;
  }
  // pinned memory is not zeroed and small blocks are recycled: a stale completion word equal to the first
  // expected sequence number (1) would end the first wait before the kernel ran
  std::memset(pin, 0, kBytes);
  seq = 0;
  return hipSuccess;
}

void HostBuf::release() {
  if (pin) (void)hipHostFree(pin);
  if (dev) (void)hipFree(dev);
  pin = map = dev = nullptr;
}

void HostBuf::put_inputs(const HostStepArgs &a) {
  if (a.actions) std::memcpy(pin, a.actions, kActBytes);
  if (a.opp_inc) std::memcpy(pin + kActBytes, a.opp_inc, kIncBytes);
}

StepIO HostBuf::io(uint8_t *base, bool actions, bool opp_inc, int flags) const {
  StepIO s{};
  s.actions = actions ? (const float *)base : nullptr;
  s.opp_inc = opp_inc ? (const double *)(base + kActBytes) : nullptr;
  uint8_t *o = base + kInBytes;
  s.obs = (float *)(o + kObs);
  s.obs2 = (float *)(o + kObs2);
  s.done = o + kDone;
  s.record = (double *)(o + kRec);
  s.flags = flags;
  return s;
}

// ------------------------------------------------------------------------------------------------ StepServer
bool StepServer::init(int device, HostBuf *buf, long wait_ms) {
  int khz = 0;
  if (hipEventCreateWithFlags(&after_, hipEventDisableTiming) != hipSuccess ||
      hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || khz <= 0) {
    destroy();
    return false;
  }
  device_ = device;
  buf_ = buf;
  wait_ = std::chrono::milliseconds(wait_ms);
  idle_ticks_ = (unsigned long long)khz * kSrvIdleMs;
  life_ticks_ = (unsigned long long)khz * kSrvLifeMs;
  return true;
}

void StepServer::destroy() {
  if (after_) (void)hipEventDestroy(after_);
  after_ = nullptr;
}

int StepServer::acquire() {
  SrvSlot &slot = srv_slot(device_);
  if (slot.owner && slot.owner != this) {
    const int rc = slot.owner->stop("hk_step_host: another context");
    if (rc != HK_OK) return rc;
  }
  // A server that has idled or lived for half its limits may be about to exit on its own: replace it now rather
  // than post a request it could miss (a missed request is still served: see await).
  const auto now = Clock::now();
  if (state_ == Abandoned || (state_ == Running && (now - last_ > std::chrono::microseconds(kSrvIdleMs * 500) ||
                                                    now - started_ > std::chrono::milliseconds(kSrvLifeMs / 2))))
    return stop("hk_step_host");
  return HK_OK;
}

uint64_t StepServer::post(int flags, bool actions, bool opp_inc) {
  volatile int32_t *args = reinterpret_cast<volatile int32_t *>(buf_->pin + HostBuf::kArgsOff);
  args[0] = flags;
  args[1] = actions ? 1 : 0;
  args[2] = opp_inc ? 1 : 0;
  const uint64_t seq = ++buf_->seq;
  std::atomic_thread_fence(std::memory_order_release);
  *req_word() = seq;  // the request: every input and argument word is written first
  return seq;
}

// start a server, ordered after the work already on the caller's stream (e.g. a reset)
hipError_t StepServer::start(const DevState &s, const KCfg &cfg, hipStream_t after) {
  SrvSlot &slot = srv_slot(device_);
  hipError_t e = hipSuccess;
  if (!slot.stream && (e = hipStreamCreateWithFlags(&slot.stream, hipStreamNonBlocking)) != hipSuccess) return e;
  HostServer hs{};
  hs.req = reinterpret_cast<const unsigned long long *>(buf_->map + HostBuf::kReqOff);
  hs.done = reinterpret_cast<unsigned long long *>(buf_->map + HostBuf::kDoneOff);
  hs.args = reinterpret_cast<const int32_t *>(buf_->map + HostBuf::kArgsOff);
  hs.idle_ticks = idle_ticks_;
  hs.life_ticks = life_ticks_;
  if ((e = hipEventRecord(after_, after)) != hipSuccess ||
      (e = hipStreamWaitEvent(slot.stream, after_, 0)) != hipSuccess ||
      (e = launch_host_server(s, cfg, buf_->io(buf_->map, true, true, 0), hs, slot.stream)) != hipSuccess)
    return e;
  stream_ = slot.stream;
  slot.owner = this;
  state_ = Running;
  started_ = Clock::now();
  return hipSuccess;
}

// Wait for the answer to request `seq`.  The wait is bounded: the slot's lock is held here, so a server
// that never starts (the caller's stream blocked) must not hold every other facade on this device.  Past the limit
// the request is withdrawn and the server abandoned; the call fails with HK_E_DEVICE.
int StepServer::await(uint64_t seq) {
  const auto deadline = Clock::now() + wait_;
  hipError_t e = hipSuccess;
  switch (wait_word(buf_->done_word(), seq, stream_, &deadline, &e)) {
    case Wait::Idle:  // it exited (idle / life limit) before it saw this request, which stays posted
      retire();
      return kRestart;
    case Wait::Error:
      retire();
      return hipfail(e, "hk_step_host: step server");
    case Wait::Deadline:
      std::atomic_thread_fence(std::memory_order_release);
      *req_word() = kServerQuit;
      if (*buf_->done_word() == seq) break;  // answered while the request was being withdrawn
      // a server that took the request in this window still steps once: include/hockey.h states the contract
      abandon();
      return fail(HK_E_DEVICE, "hk_step_host: the step server did not answer within the wait limit (is the "
                               "calling stream blocked?); reset or set the state before the next step%s");
    case Wait::Answered:
      break;
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  last_ = Clock::now();
  return HK_OK;
}

// Tell the server to quit and wait, at most the wait limit, for its stream: every request it was given has been
// answered or withdrawn, so the next server starts idle.
int StepServer::stop(const char *who) {
  if (state_ == Stopped) return HK_OK;
  std::atomic_thread_fence(std::memory_order_release);
  *req_word() = kServerQuit;
  const auto deadline = Clock::now() + wait_;
  hipError_t e = hipSuccess;
  switch (wait_word(nullptr, 0, stream_, &deadline, &e)) {
    case Wait::Deadline:
      abandon();
      return fail(HK_E_DEVICE, "%s: the step server's stream is still busy after the wait limit (is the stream "
                               "it was started from blocked?)", who);
    case Wait::Error:
      retire();
      return hipfail(e, (std::string(who) + ": step server").c_str());
    default:
      retire();
      return HK_OK;
  }
}

// the server's stream is idle (or failed): nothing of this context is on it any more
void StepServer::retire() {
  SrvSlot &slot = srv_slot(device_);
  if (slot.owner == this) slot.owner = nullptr;
  if (stream_ != slot.stream) {  // abandoned earlier: the slot went on with a stream of its own
    if (slot.stream) (void)hipStreamDestroy(stream_);
    else slot.stream = stream_;
  }
  stream_ = nullptr;
  *req_word() = buf_->seq;
  state_ = Stopped;
}

// give up waiting: the quit word stays posted, the slot is free for other contexts and gets a fresh stream
void StepServer::abandon() {
  SrvSlot &slot = srv_slot(device_);
  if (slot.owner == this) slot.owner = nullptr;
  if (slot.stream == stream_) slot.stream = nullptr;
  state_ = Abandoned;
}

// ------------------------------------------------------------------------------------------------ HostStep
int HostStep::ensure_buffers() {
  if (buf.pin) return HK_OK;
  const char *v = std::getenv("HK_STEP_HOST_STAGED");
  staged = v && v[0] == '1';
  const char *sv = std::getenv("HK_STEP_HOST_SERVER");
  served = !staged && !(sv && sv[0] == '0');
  const char *wv = std::getenv("HK_STEP_HOST_WAIT_MS");
  const long wait_ms = wv ? std::strtol(wv, nullptr, 10) : 0;
  const hipError_t e = buf.alloc(staged);
  if (e != hipSuccess) return hipfail(e, "hk_step_host: buffer allocation");
  if (served) served = srv.init(device, &buf, wait_ms > 0 ? wait_ms : kSrvWaitMs);
  return HK_OK;
}

int HostStep::step(const DevState &s, const KCfg &cfg, const HostStepArgs &a) {
  const int rc = ensure_buffers();
  if (rc != HK_OK) return rc;
  return served ? step_via_server(s, cfg, a) : staged ? step_staged(s, cfg, a) : step_via_launch(s, cfg, a);
}

int HostStep::step_via_server(const DevState &s, const KCfg &cfg, const HostStepArgs &a) {
  std::lock_guard<std::mutex> lk(srv_slot(device).mu);
  int rc = srv.acquire();
  if (rc != HK_OK) return rc;
  buf.put_inputs(a);
  const uint64_t seq = srv.post(a.flags, a.actions != nullptr, a.opp_inc != nullptr);
  for (int launches = 0;;) {
    if (srv.state() == StepServer::Stopped) {
      if (++launches > 2) return fail(HK_E_DEVICE, "hk_step_host: the step server exits without serving%s");
      const hipError_t e = srv.start(s, cfg, a.st);
      if (e != hipSuccess) return hipfail(e, "hk_step_host: server launch");
    }
    if ((rc = srv.await(seq)) == HK_OK) break;
    if (rc != StepServer::kRestart) return rc;
  }
  buf.get_record(a.out);
  return HK_OK;
}

// The kernel stores the launch's sequence number into the completion word in the mapped buffer after its last output
// store, and the host waits on that word instead of synchronising the stream.
int HostStep::step_via_launch(const DevState &s, const KCfg &cfg, const HostStepArgs &a) {
  buf.put_inputs(a);
  StepIO io = buf.io(buf.map, a.actions != nullptr, a.opp_inc != nullptr, a.flags);
  io.done_word = reinterpret_cast<unsigned long long *>(buf.map + HostBuf::kDoneOff);
  io.done_seq = ++buf.seq;
  hipError_t e = launch_step(s, cfg, io, 1, a.st);
  if (e != hipSuccess) return hipfail(e, "hk_step_host: launch");
  switch (wait_word(buf.done_word(), io.done_seq, a.st, nullptr, &e)) {
    case Wait::Answered:
      break;
    case Wait::Error:
      return hipfail(e, "hk_step_host: step kernel");
    default:
      return fail(HK_E_DEVICE, "hk_step_host: the step finished without its completion word%s");
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  buf.get_record(a.out);
  return HK_OK;
}

int HostStep::step_staged(const DevState &s, const KCfg &cfg, const HostStepArgs &a) {
  const StepIO io = buf.io(buf.dev, a.actions != nullptr, a.opp_inc != nullptr, a.flags);
  buf.put_inputs(a);
  hipError_t e = hipSuccess;
  if ((a.actions || a.opp_inc) &&
      (e = hipMemcpyAsync(buf.dev, buf.pin, HostBuf::kInBytes, hipMemcpyHostToDevice, a.st)) != hipSuccess)
    return hipfail(e, "hk_step_host: H2D");
  if ((e = launch_step(s, cfg, io, 1, a.st)) != hipSuccess) return hipfail(e, "hk_step_host: launch");
  if ((e = hipMemcpyAsync(buf.pin + HostBuf::kInBytes, buf.dev + HostBuf::kInBytes, HK_HOST_RECORD_BYTES,
                          hipMemcpyDeviceToHost, a.st)) != hipSuccess)
    return hipfail(e, "hk_step_host: D2H");
  if ((e = hipStreamSynchronize(a.st)) != hipSuccess) return hipfail(e, "hk_step_host: sync");
  buf.get_record(a.out);
  return HK_OK;
}

int HostStep::quiesce(const char *who) {
  if (!served) return HK_OK;  // this context never started a server (served is set by its own thread)
  std::lock_guard<std::mutex> lk(srv_slot(device).mu);
  return srv.stop(who);
}

bool HostStep::release() {
  if (srv.state() != StepServer::Stopped) return false;
  srv.destroy();
  buf.release();
  return true;
}

}  // namespace hk
