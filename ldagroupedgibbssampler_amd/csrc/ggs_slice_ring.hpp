// ggs_slice_ring.hpp -- the per-wave LDS ring through which the z kernels gather 64 phiT rows per chunk (or per step), a
// slice of 128 bytes per row at a time, by LDS-DMA.  One copy of the layout contract for z_sliced_kernel and
// z_sliced32_kernel (ggs_z_sliced.hpp), pcgs_sliced_kernel, polyaurn_sliced_kernel, pcgs_z_kernel and polyaurn_z_kernel
// (ggs_z_pcgs.hpp), z_stream_kernel and z_stream1_kernel (ggs_z_stream.hpp).  Plain functions: the ring's state (the
// slot of the current slice, the row addresses of this chunk and the next) stays in each kernel's own loop.
//
// DMA shape: one global_load_lds_dwordx4 wave-instruction fills 1 KiB = 8 rows x 128 B, lane l
// -> row 8m + l/8, LDS slot l%8.  Slot j of row r holds source unit (j - r/2) mod 8 (a per-row
// rotation chosen through the per-lane SOURCE address), so lane t's 16-byte read of unit u, at
// slot (u + t/2) mod 8 of row t, is bank-conflict free across the wave.  Per chunk every lane
// computes its 8 source row addresses once; the slice offset is either added to them (the slice a run-time
// value) or the DMA instruction's immediate (the slice a template argument)
// -- which the hardware adds to the LDS destination as well as to the global source, hence the
// "- s*128" on the destination and a ring that does not start at LDS address 0.  The ring slot
// is wave-uniform and reaches M0 through scalar registers.
// Lanes with nothing useful to fetch (rows past the chunk, units past the row) read whatever
// finite bytes sit there (word 0's row; the next row's first entries; the zeroed tail pad of
// phiT): those scores are multiplied by theta = 0 or belong to lanes that store nothing.
#pragma once
#include "ggs_z_kernel.hpp"

namespace ggs {

constexpr int kSliceUnits = 8;            // 16-byte units per row per slice
constexpr int kSliceBytes = 64 * 128;     // 64 rows x 128 B: one ring slot

// ---- write side.  The lane's 8 DMA source addresses (m = 0..7): row 8m + lane/8 of the chunk, whose word id lane
// `row` holds in w, unit (lane%8 - row/2) mod 8 of slice 0.  `mask` is applied AFTER the shuffle (the sliced kernels keep
// the token's theta row above bit kSlotShift of w and pass (1 << kSlotShift) - 1; rows past the chunk hold word 0).
__device__ __forceinline__ void ring_row_addresses(const unsigned char *base, const size_t rowbytes, const int w, const int mask,
                                                   const int lane, const unsigned char *(&ra)[8]) {
  const int lrow = lane >> 3, lslot = lane & 7;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int row = 8 * m + lrow;
    const int wm = __shfl(w, row) & mask;
    ra[m] = base + (size_t)wm * rowbytes + (size_t)(((lslot - (row >> 1)) & 7) << 4);
  }
}
__device__ __forceinline__ void ring_row_addresses(const unsigned char *base, const size_t rowbytes, const int w, const int lane,
                                                   const unsigned char *(&ra)[8]) {
  ring_row_addresses(base, rowbytes, w, -1, lane, ra);
}
// Slice s of the rows `ra` into ring slot `slot`: 8 DMA instructions, issued in order.  s a template argument: the slice
// offset is the instruction's immediate and `ring` must lie at least slices * 128 bytes above LDS address 0.
template <int s>
__device__ __forceinline__ void ring_issue(unsigned char *ring, const int slot, const unsigned char *const (&ra)[8]) {
#pragma unroll
  for (int m = 0; m < 8; ++m)
    __builtin_amdgcn_global_load_lds((glb_cvoid_t *)ra[m],
                                     (lds_void_t *)(ring + slot * kSliceBytes + m * 1024 - s * 128), 16, s * 128, 0);
}
// ... s a run-time value: the offset goes to the source address
__device__ __forceinline__ void ring_issue(unsigned char *ring, const int s, const int slot, const unsigned char *const (&ra)[8]) {
  const size_t off = (size_t)s * 128;
#pragma unroll
  for (int m = 0; m < 8; ++m)
    __builtin_amdgcn_global_load_lds((glb_cvoid_t *)(ra[m] + off),
                                     (lds_void_t *)(ring + slot * kSliceBytes + m * 1024), 16, 0, 0);
}

// ---- read side.  Lane t's row of slot 0, its rotation (the one the write side chose for row t) and the byte offset of
// unit u of the row under that rotation.
__device__ __forceinline__ const unsigned char *ring_lane_row(const unsigned char *ring, const int lane) { return ring + lane * 128; }
__device__ __forceinline__ int ring_lane_rotation(const int lane) { return lane >> 1; }
__device__ __forceinline__ int ring_unit_offset(const int u, const int rot) { return ((u + rot) & 7) << 4; }

// ---- completion.  LDS-DMA completion is tracked by vmcnt in issue order, 8 DMAs per slice: "all but the youngest 8n
// have landed" means the slice issued n slices ago is in LDS.  The waves of a workgroup never meet in a chunk loop: no
// hardware barrier, the "memory" clobber keeps every LDS read below the wait.
template <int n>
__device__ __forceinline__ void ring_wait_all_but() {
  static_assert(n >= 0 && 8 * n <= 63, "vmcnt is a 6-bit count: at most 7 slices in flight behind the one waited for");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(8 * n) : "memory");
}
// n a run-time value, 0 <= n <= kMax (the caller clamps; any other n waits for every DMA, which is always safe)
template <int kMax>
__device__ __forceinline__ void ring_wait_all_but(const int n) {
  if constexpr (kMax == 0) ring_wait_all_but<0>();
  else if (n == kMax) ring_wait_all_but<kMax>();
  else ring_wait_all_but<kMax - 1>(n);
}
// Slice s of a chunk of NS slices with kAhead slices kept in flight behind the one being used: kAhead slices were issued
// after it (the last of them from the next chunk, has1), except at the tail of the last chunk, where fewer follow.
template <int kAhead, int NS, int s>
__device__ __forceinline__ void ring_wait(const bool has1) {
  if constexpr (s + kAhead < NS) {
    ring_wait_all_but<kAhead>();
  } else {
    if (has1) ring_wait_all_but<kAhead>();
    else ring_wait_all_but<NS - 1 - s>();
  }
}

// ---- release: what must hold of a slot's LDS reads before the next step's DMA may refill it.  Two rules are in use,
// and each kernel keeps the one it was measured and tested with:
//   ring_release_returned   z_sliced32_kernel and z_sliced_kernel (one loop: cold_chunk_loop, ggs_z_sliced.hpp)
//   ring_release_issued     pcgs_sliced_kernel, polyaurn_sliced_kernel, pcgs_z_kernel, polyaurn_z_kernel, z_stream_kernel,
//                           z_stream1_kernel
// DESIGN.md section 5 on the float32 kernel: "the ring slot's LDS reads must have *returned*, not only been issued, before
// the next DMA may refill the slot -- beside the table waves of the fused form an L2 hit overwrote a slot under queued
// reads (wrong draws in the fused form only); the float32 kernel waits `lgkmcnt(0)` at the end of every slice."  How it
// comes about: issued is not enough because the scheduler may sink the arithmetic (and the compiler's wait for these
// reads) behind that DMA, and beside the table waves the reads queue long enough for an L2 hit to land first.
// No argument that "issued" suffices is on record for the six fp64 kernels that keep it: they pass their tests with it, and
// nothing says why the float32 kernel's hazard cannot reach them (open question).
__device__ __forceinline__ void ring_release_returned() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void ring_release_issued() { asm volatile("" ::: "memory"); }

}  // namespace ggs
