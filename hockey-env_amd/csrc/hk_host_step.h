// hk_host_step.h -- hk_step_host's host side: the pinned buffer (HostBuf), the resident step server's protocol and
// state (StepServer) and the three step paths (HostStep::step).  hk_capi.cpp validates and calls in here.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstring>
#include <mutex>

#include "../../include/hockey.h"
#include "hk_kernels.h"

namespace hk {

constexpr int kMaxDevices = 64;  // one step-server slot per device id; hk_create rejects an id beyond it

// status plus thread-local message (hk_last_error); defined in hk_capi.cpp
int fail(int code, const char *fmt, const char *a = "", long long b = 0);
int hipfail(hipError_t e, const char *where);

// one hk_step_host call's arguments (include/hockey.h)
struct HostStepArgs {
  const float *actions;
  const double *opp_inc;
  int flags;
  void *out;
  hipStream_t st;
};

// The context's pinned, mapped, coherent host buffer and the only place that knows its layout (one arena):
//   inputs   f32[8] actions, f64[2] phase increments
//   record   HK_HOST_RECORD_BYTES: obs f32[18], obs2 f32[18], done u8 + 7 pad, record f64[16]
//   then, each on a 64-B line of its own: the completion word, the server's request word, its argument words
// The step kernel reads the inputs and writes the record through `map` (the buffer's device address), so a step
// costs no copy command; HK_STEP_HOST_STAGED=1 goes through the device twin `dev` instead (A/B timing).
struct HostBuf {
  static constexpr size_t kActBytes = 8 * 4, kIncBytes = 2 * 8, kInBytes = kActBytes + kIncBytes;
  static constexpr size_t kObs = 0, kObs2 = 72, kDone = 144, kRec = 152;
  static_assert(kRec + 16 * 8 == HK_HOST_RECORD_BYTES, "hk_step_host record layout");
  static constexpr size_t kLine = 64;
  static constexpr size_t kDoneOff = (kInBytes + HK_HOST_RECORD_BYTES + kLine - 1) & ~(kLine - 1);
  static constexpr size_t kReqOff = kDoneOff + kLine, kArgsOff = kDoneOff + 2 * kLine, kBytes = kDoneOff + 3 * kLine;

  uint8_t *pin = nullptr, *map = nullptr, *dev = nullptr;
  uint64_t seq = 0;  // steps requested so far: the value the completion word takes when the last one is done

  hipError_t alloc(bool staged);
  void release();
  void put_inputs(const HostStepArgs &a);
  void get_record(void *out) const { std::memcpy(out, pin + kInBytes, HK_HOST_RECORD_BYTES); }
  volatile uint64_t *done_word() const { return reinterpret_cast<volatile uint64_t *>(pin + kDoneOff); }
  // one step's StepIO on `base` (map or dev); an input that is not given is a null pointer
  StepIO io(uint8_t *base, bool actions, bool opp_inc, int flags) const;
};

// One resident step server per context, at most one RUNNING per device and process: SrvSlot (hk_host_step.cpp)
// holds the device's server stream and the server that owns it, and its mutex guards every member here.
//   Stopped    nothing of this context is on a server stream
//   Running    a server kernel is queued or resident on `stream` and owns the slot
//   Abandoned  a server kernel may still be queued or resident on `stream`, but nobody waits for it: the quit word
//              stays posted (a server that starts late exits without stepping) and the slot has been released with
//              a fresh stream, so other contexts are not held up.  stop() returns it to Stopped once its stream is
//              found idle.
// Every wait is bounded by the wait limit; the request word and the slot's owner are written only here.
class StepServer {
 public:
  enum State { Stopped, Running, Abandoned };
  State state() const { return state_; }
  // false: no server for this context (its steps take the launch-per-step path)
  bool init(int device, HostBuf *buf, long wait_ms);
  void destroy();
  // hand the slot over from another context's server and retire an abandoned or soon-to-expire one of our own
  int acquire();
  uint64_t post(int flags, bool actions, bool opp_inc);
  hipError_t start(const DevState &s, const KCfg &cfg, hipStream_t after);
  enum { kRestart = 1 };  // await: the server exited on its own limits before this request; start another
  int await(uint64_t seq);
  int stop(const char *who);

 private:
  void retire();
  void abandon();
  volatile uint64_t *req_word() const { return reinterpret_cast<volatile uint64_t *>(buf_->pin + HostBuf::kReqOff); }

  State state_ = Stopped;
  int device_ = 0;
  HostBuf *buf_ = nullptr;
  hipStream_t stream_ = nullptr;  // where this context's server was launched (Running / Abandoned)
  hipEvent_t after_ = nullptr;
  std::chrono::milliseconds wait_{0};
  std::chrono::steady_clock::time_point started_, last_;
  unsigned long long idle_ticks_ = 0, life_ticks_ = 0;
};

// hk_step_host's per-context state (a member of the C ABI's context)
struct HostStep {
  int device = 0;
  HostBuf buf;
  StepServer srv;
  bool staged = false, served = false;  // the step path, picked from the environment at the first step

  int step(const DevState &s, const KCfg &cfg, const HostStepArgs &a);
  // stop the step server before any other work of the context (a no-op for a context that never started one)
  int quiesce(const char *who);
  // free everything; false (and nothing is freed) while a server kernel may still touch the buffers
  bool release();

 private:
  int ensure_buffers();
  int step_via_server(const DevState &s, const KCfg &cfg, const HostStepArgs &a);
  int step_via_launch(const DevState &s, const KCfg &cfg, const HostStepArgs &a);
  int step_staged(const DevState &s, const KCfg &cfg, const HostStepArgs &a);
};

}  // namespace hk
