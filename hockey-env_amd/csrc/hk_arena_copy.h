// hk_arena_copy.h -- exact per-arena copies: every word of an arena that outlives a step, between two views.
//
// A VIEW is a DevState-shaped set of arrays plus its arena count: a live context (n = N) or a snapshot blob (n =
// the blob's row count, the arrays packed in one allocation in the order f, i, phase, man, each 16-B aligned).
// copy_arena moves
//   f[NFF]            body state, centres of mass, sleep times, the puck's pending force
//   i[NPW]            the packed int words: touching / enabled / awake bits, done, winner, one_starts, has_puck,
//                     max_t, time and the episode / step words that key the device Philox draws
//   phase[3]          the BasicOpponent phase rows
//   man[NSOLID][NMF]  ALL manifold records with their warm-start impulses, touching or not: begin-touching reads
//                     the stored record, so a stale one is state too, and the dense copy is what "exact" means
// The step's other memory is per-step scratch and is not copied: DevState::ws (HbmSlots) is written by set_pair /
// the slot initialisation of a solve before that solve reads it, and the LDS rows (TOI alphas, static alpha0, TOI
// counts) are valid only under toiflag, which every step starts at 0, or are cleared at the start of solve_toi.
// Counters belong to the context, not to the arena.
//
// One source for the gfx950 kernel (hk_arena_copy.hip: lane per entry for the rows, four lanes per 64-B record for
// the manifolds) and for the host build (hostcheck/hk_hostcheck.cpp: copy_arena looped on the CPU).
#pragma once
#include "hk_kernels.h"

namespace hk {

constexpr int kPhaseRows = 3;
constexpr int kRecQuads = NMF / 4;  // a manifold record is four 16-B quads (hk_kernels.h)
// bytes of one arena in a view: 116 + 24 + 24 + 1600 with today's enums
constexpr int64_t kArenaBytes = (int64_t)NFF * 4 + NPW * 4 + kPhaseRows * 8 + (int64_t)NSOLID * NMF * 4;

struct ArenaView {
  float *f;       // [NFF][n]
  int32_t *i;     // [NPW][n]
  double *phase;  // [kPhaseRows][n]
  float *man;     // [NSOLID][n][NMF], 16-B aligned
  int64_t n;
};

inline ArenaView view_of(const DevState &s) { return ArenaView{s.f, s.i, s.phase, s.man, s.n}; }

// blob layout of m rows: section offsets (bytes), each rounded up to 16
struct BlobLayout {
  int64_t f, i, phase, man, bytes;
};
inline BlobLayout blob_layout(int64_t m) {
  auto up = [](int64_t x) { return (x + 15) & ~(int64_t)15; };
  BlobLayout L;
  L.f = 0;
  L.i = up(L.f + (int64_t)NFF * 4 * m);
  L.phase = up(L.i + (int64_t)NPW * 4 * m);
  L.man = up(L.phase + (int64_t)kPhaseRows * 8 * m);
  L.bytes = L.man + (int64_t)NSOLID * NMF * 4 * m;
  return L;
}
inline ArenaView blob_view(void *blob, int64_t m) {
  const BlobLayout L = blob_layout(m);
  char *b = static_cast<char *>(blob);
  return ArenaView{reinterpret_cast<float *>(b + L.f), reinterpret_cast<int32_t *>(b + L.i),
                   reinterpret_cast<double *>(b + L.phase), reinterpret_cast<float *>(b + L.man), m};
}

// entry e of a copy list: its destination and source arena (a null list is the identity).  False, and nothing is
// to be copied, when either index is outside its view.
HK_DEV bool copy_entry(const ArenaView &dst, const int64_t *dst_idx, const ArenaView &src, const int64_t *src_idx,
                       int64_t e, int64_t &di, int64_t &si) {
  di = dst_idx ? dst_idx[e] : e;
  si = src_idx ? src_idx[e] : e;
  return di >= 0 && di < dst.n && si >= 0 && si < src.n;
}

// the scalar rows of one arena
HK_DEV void copy_arena_rows(const ArenaView &dst, int64_t di, const ArenaView &src, int64_t si) {
  float fw[NFF];
  int32_t iw[NPW];
  double ph[kPhaseRows];
#pragma unroll
  for (int k = 0; k < NFF; ++k) fw[k] = src.f[(int64_t)k * src.n + si];
#pragma unroll
  for (int k = 0; k < NPW; ++k) iw[k] = src.i[(int64_t)k * src.n + si];
#pragma unroll
  for (int k = 0; k < kPhaseRows; ++k) ph[k] = src.phase[(int64_t)k * src.n + si];
#pragma unroll
  for (int k = 0; k < NFF; ++k) dst.f[(int64_t)k * dst.n + di] = fw[k];
#pragma unroll
  for (int k = 0; k < NPW; ++k) dst.i[(int64_t)k * dst.n + di] = iw[k];
#pragma unroll
  for (int k = 0; k < kPhaseRows; ++k) dst.phase[(int64_t)k * dst.n + di] = ph[k];
}

// quad q of solid pair p's manifold record: one 16-B load and one 16-B store.  A native vector type (clang and
// gcc): a chunk of them stays in registers
typedef uint32_t CopyQuad __attribute__((vector_size(16)));
HK_DEV const CopyQuad *man_quad(const ArenaView &v, int p, int64_t a, int q) {
  return reinterpret_cast<const CopyQuad *>(v.man + ((int64_t)p * v.n + a) * NMF) + q;
}
// quad q of every record of one arena, kManChunk loads in flight before their stores
constexpr int kManChunk = 5;
HK_DEV void copy_arena_quads(const ArenaView &dst, int64_t di, const ArenaView &src, int64_t si, int q) {
#pragma unroll
  for (int p0 = 0; p0 < NSOLID; p0 += kManChunk) {
    CopyQuad r[kManChunk];
#pragma unroll
    for (int j = 0; j < kManChunk; ++j)
      if (p0 + j < NSOLID) r[j] = *man_quad(src, p0 + j, si, q);
#pragma unroll
    for (int j = 0; j < kManChunk; ++j)
      if (p0 + j < NSOLID) *const_cast<CopyQuad *>(man_quad(dst, p0 + j, di, q)) = r[j];
  }
}

// everything of arena si of src into arena di of dst
HK_DEV void copy_arena(const ArenaView &dst, int64_t di, const ArenaView &src, int64_t si) {
  copy_arena_rows(dst, di, src, si);
  for (int q = 0; q < kRecQuads; ++q) copy_arena_quads(dst, di, src, si, q);
}

// hk_arena_copy.hip.  `bad` is the destination context's HK_CNT_BAD_INDEX word.
hipError_t launch_copy_arenas(const ArenaView &dst, const int64_t *dst_idx, const ArenaView &src,
                              const int64_t *src_idx, int64_t m, unsigned long long *bad, hipStream_t st);

}  // namespace hk
