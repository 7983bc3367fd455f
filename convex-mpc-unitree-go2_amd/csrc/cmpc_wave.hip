// cmpc_wave.hip -- batched convex-MPC contact-force QP solver for MI355X (gfx950):
// ONE WAVEFRONT PER QP INSTANCE.
//
// Each 64-lane wave solves one QP of the reference's centroidal MPC
// (convex_mpc/centroidal_mpc.py:69-359) with no workgroup barrier anywhere: the workgroup is the
// wave, all cross-lane traffic is wave-ordered LDS or DPP, and a CU keeps 8 independent QPs in
// flight (2 per SIMD) so one QP's latency is hidden behind another's MFMA/VALU work.
// Algorithm (DESIGN.md "Kernel"):
//
//   1. Condense the horizon onto the free (stance) forces straight into register tiles:
//      H = sum_t G_t' Q2 G_t + diag(R) + shift with G_t = A G_{t-1} + (step t's new columns),
//      each product three v_mfma_f32_16x16x4_f32 (K = 12 states) whose accumulator is the
//      tile itself (condense_tiles_fwd); small batches use the block-row form
//      H_ij = C_i' A^{i-j} B_j, P_i = Q2 + A'P_{i+1}A (condense_tiles_bc).  Lane (g, c) holds
//      rows 4g..4g+3, column c of every lower-triangle 16x16 tile (f4 per tile, in registers).
//   2. Factor H + diag(R) + shift in registers by the BLOCK sweep operator, four pivots at a
//      time: S <- S - P^ D^-1 P^' (P^ = the four pivot columns with the pivot block minus I),
//      then -2 on the four pivot diagonals; the rank-4 update of each tile is ONE MFMA
//      (A = -Y rows, B = diag(1/dl) Y' columns, Y = P^ L^-T from the 4x4 LDL' of the pivot
//      block, factored redundantly per lane: pivot_block); pivot columns go through a 4-column
//      LDS panel.  Swept only on the tiles right of the pivots, this leaves a block LDL'
//      factorization (ldl_tiles), applied by two block substitutions (ldl_apply); the team
//      kernel (cmpc_team.hip) sweeps every tile into the explicit inverse instead.
//   3. ADMM (OSQP iteration, A = I) on the free forces, lane t owning stance triple t
//      {fz >= fz_min, |fx| <= mu fz, |fy| <= mu fz} (closed-form projection).  Defect-correction
//      x-update x~ = x + M(rho(z - x) - grad f(x) - y): M (the fp32 factors) preconditions, grad f
//      comes from the error-coordinate rollout/adjoint (e_{k+1} = A e_k + B_k u_k + d_k).
//   4. Active-set polish once the face pattern is stable: reduced basis u = T v + t0, condense
//      + factor again (the ADMM factors are parked in a per-wave global slab), refine with the
//      exact gradient, KKT check, primal-dual repairs of the face set.
//
// Instances are binned by free-variable count (NC in {96,128,160,192}, a multiple of 16);
// each bin runs a persistent kernel whose waves pull instance ids from a device-side queue.
//
// The source by phase, each file including what it uses: cmpc_wave_prims.h (wave primitives),
// cmpc_instance.h (constants, LDS image), cmpc_condense.h (1), cmpc_factor.h (2),
// cmpc_gradient.h (grad f), cmpc_polish.h (4), cmpc_team.hip (W waves per QP), cmpc_solve.h
// (the phases of one instance and its driver); this file holds the kernels.
// It is compiled as part of cmpc_host.hip (single translation unit).
#include "cmpc_device.h"
#include "cmpc_solve.h"

namespace cmpc {

// LDS slot: each class kernel's allocation is padded to a multiple of kLdsSlot, so that an
// NC >= 160 wave's block (2 slots, 39,936 B) is exactly two NC <= 128 blocks (1 slot; 19,632 B
// used) and the 160 KiB of a CU hold 8 of one or 4 of the other (every power-of-two allocation
// granule up to 4 KiB rounds both alike).  When the NC >= 160 class runs first and its waves
// exit one by one, the two NC <= 128 waves that take over each freed SIMD then also fit into
// the LDS it freed: unpadded (27,056 B), the CU's LDS fragmented and the NC <= 128 kernel ran
// with ~1,550 of its 2,048 waves resident for the rest of the step (tools/shard_anatomy.py).
constexpr size_t kLdsSlot = 19968;

// LDS image of a group kernel's bins (NCB = 0: a single-bin kernel)
template <int NC>
constexpr size_t smem_size() {
  if constexpr (NC == 0) return 0;
  else return sizeof(Smem<NC>);
}

// One persistent kernel per register class: bins NCA and NCB share the occupancy (two waves per
// SIMD for NC <= 128, one for NC >= 144), so one kernel serves both, draining the larger bin
// first (its instances are the slower ones: hardest first shortens the batch tail).  NCB = 0:
// one bin (the NC = 192 kernel).  Kernels submitted concurrently on their own streams (the
// caller's + two plan streams) stay within the device's hardware queues, so the classes really
// overlap.
template <int NCA, int NCB>
__global__ void __launch_bounds__(64, Cfg<NCA>::WPE)
    solve_group_kernel(KParams P, Inputs in, Outputs out, const int* __restrict__ list_a,
                       const int* __restrict__ list_b, const int* __restrict__ counts,
                       int* __restrict__ heads, int qa, float* __restrict__ work,
                       size_t slab) {
  static_assert(NCB == 0 || Cfg<NCA>::WPE == Cfg<NCB>::WPE, "a group shares one occupancy class");
  constexpr size_t kImg = smem_size<NCA>() > smem_size<NCB>() ? smem_size<NCA>() : smem_size<NCB>();
  constexpr size_t kBytes = kLdsSlot ? (kImg + kLdsSlot - 1) / kLdsSlot * kLdsSlot : kImg;
  static_assert(!kLdsSlot || 4 * kBytes <= 160 * 1024, "one wave per SIMD must fit the CU's LDS");
  // the two-wave class must stay within ONE slot: a layout change that rounds it up to two
  // would halve its waves per CU (and break the heavy-first hand-over of freed LDS)
  static_assert(!kLdsSlot || Cfg<NCA>::WPE == 1 || kImg <= kLdsSlot, "NC <= 128 image exceeds the LDS slot");
  static_assert(Cfg<NCA>::WPE * 4 * kBytes <= 160 * 1024, "the class's waves per CU must fit the LDS");
  __shared__ __attribute__((aligned(16))) unsigned char raw[kBytes];
  float* park = work + (size_t)blockIdx.x * slab;
#ifdef CMPC_STAMPS
  // st[] is the first member of every Smem<NC>: one set of totals for the wave
  Smem<NCA>& s0 = *reinterpret_cast<Smem<NCA>*>(raw);
  if (threadIdx.x < 32) s0.st[threadIdx.x] = 0;
#endif
  drain_bin<NCA, 1>(*reinterpret_cast<Smem<NCA>*>(raw), P, in, out, list_a, counts + qa,
                         heads + qa, park);
  if constexpr (NCB > 0) {
    drain_bin<NCB, 1>(*reinterpret_cast<Smem<NCB>*>(raw), P, in, out, list_b,
                           counts + qa - 1, heads + qa - 1, park);
  }
#ifdef CMPC_STAMPS
  WSYNC();
  if (threadIdx.x < 32) atomicAdd(&g_stamps[threadIdx.x], s0.st[threadIdx.x]);
#endif
}

// Team mode (cmpc_team.hip): one workgroup of W waves per QP, one kernel for all five bins
// (heaviest first: the slow instances start first).  Wave 0 leads (drain loop +
// solve_instance), waves 1..W-1 serve its matrix commands; the tiles are split W ways, so
// every bin fits the same register class and a small batch needs one launch on the caller's
// stream, no fork/join.  OCC = workgroups per CU: 2 (<= 256 registers per lane) for B > CUs,
// 1 (<= 512: no spills) when every QP has a CU of its own.
template <int W, int OCC>
__global__ void __launch_bounds__(64 * W, OCC)
    solve_team_kernel(KParams P, Inputs in, Outputs out, const int* __restrict__ lists,
                      int64_t stride, const int* __restrict__ counts, int* __restrict__ heads,
                      float* __restrict__ work, size_t slab) {
  constexpr size_t kS0 = sizeof(Smem<192>);
  static_assert(sizeof(Smem<192>) >= sizeof(Smem<160>) && sizeof(Smem<160>) >= sizeof(Smem<128>) &&
                    sizeof(Smem<128>) >= sizeof(Smem<96>), "Smem grows with NC");
  constexpr size_t kS = (kS0 + 15) & ~size_t(15);
  constexpr size_t kT = sizeof(TeamSmem<192, W>);
  static_assert(sizeof(TeamSmem<192, W>) >= sizeof(TeamSmem<160, W>) &&
                    sizeof(TeamSmem<160, W>) >= sizeof(TeamSmem<128, W>) &&
                    sizeof(TeamSmem<128, W>) >= sizeof(TeamSmem<96, W>), "TeamSmem grows with NC");
  __shared__ __attribute__((aligned(16))) unsigned char raw[kS + kT];
  float* park = work + (size_t)blockIdx.x * slab;
  Smem<192>& s3 = *reinterpret_cast<Smem<192>*>(raw);
  Smem<160>& s2 = *reinterpret_cast<Smem<160>*>(raw);
  Smem<128>& s1 = *reinterpret_cast<Smem<128>*>(raw);
  Smem<96>& s0 = *reinterpret_cast<Smem<96>*>(raw);
  TeamSmem<192, W>& t3 = *reinterpret_cast<TeamSmem<192, W>*>(raw + kS);
  TeamSmem<160, W>& t2 = *reinterpret_cast<TeamSmem<160, W>*>(raw + kS);
  TeamSmem<128, W>& t1 = *reinterpret_cast<TeamSmem<128, W>*>(raw + kS);
  TeamSmem<96, W>& t0 = *reinterpret_cast<TeamSmem<96, W>*>(raw + kS);
  const int w = uniform((int)(threadIdx.x >> 6));
  int seq = 0;
#ifdef CMPC_STAMPS
  if (threadIdx.x < 32) s1.st[threadIdx.x] = 0;
#endif
  if (w == 0) {
    drain_bin<192, W>(s3, P, in, out, lists + 4 * stride, counts + 4, heads + 4, park, &t3, &seq);
    // bins 3 (NC 160) and 2 (NC 144) in the NC = 160 image (team mode pairs tile columns, so
    // TT must be even); one copy of the code
#pragma unroll 1
    for (int q = 3; q >= 2; --q)
      drain_bin<160, W>(s2, P, in, out, lists + q * stride, counts + q, heads + q, park, &t2, &seq);
    drain_bin<128, W>(s1, P, in, out, lists + stride, counts + 1, heads + 1, park, &t1, &seq);
    drain_bin<96, W>(s0, P, in, out, lists, counts, heads, park, &t0, &seq);
  } else {
    team_helpers<W, 1>(s3, t3, s2, t2, s1, t1, s0, t0, P, park, w, seq);
  }
#ifdef CMPC_STAMPS
  __syncthreads();
  if (threadIdx.x < 32) atomicAdd(&g_stamps[threadIdx.x], s1.st[threadIdx.x]);
#endif
}

// Binning of a small batch (B <= 1024) in one workgroup: counts are written, not accumulated,
// and the queue heads are zeroed here, so no memset precedes it (one launch less per solve).
__global__ void __launch_bounds__(1024) bin_small_kernel(int N, int B,
                                                         const uint8_t* __restrict__ contact,
                                                         int* __restrict__ counts,
                                                         int* __restrict__ heads,
                                                         int* __restrict__ lists, int64_t stride) {
  __shared__ int wcnt[16][kNumBins];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  int bin = -1;
  if (t < B) {
    const uint8_t* c = contact + (int64_t)t * 4 * N;
    int cnt = 0;
    for (int i = 0; i < 4 * N; ++i) cnt += c[i] != 0;
    const int nf = 3 * cnt;
    bin = kNumBins - 1;
    for (int q = 0; q < kNumBins; ++q)
      if (nf <= kBinCap[q]) { bin = q; break; }
  }
  unsigned long long mine = 0;
#pragma unroll
  for (int q = 0; q < kNumBins; ++q) {
    const unsigned long long m = __ballot(bin == q);
    if (bin == q) mine = m;
    if (lane == 0) wcnt[wv][q] = __popcll(m);
  }
  __syncthreads();
  if (bin >= 0) {
    int base = 0;
    for (int v = 0; v < wv; ++v) base += wcnt[v][bin];
    const int rank = __popcll(mine & ((1ull << lane) - 1ull));
    lists[(int64_t)bin * stride + base + rank] = t;
  }
  if (t < kNumBins) {
    int total = 0;
    for (int v = 0; v < 16; ++v) total += wcnt[v][t];
    counts[t] = total;
    heads[t] = 0;
  }
}

__global__ void __launch_bounds__(256) bin_kernel(int N, int64_t B,
                                                  const uint8_t* __restrict__ contact,
                                                  int* __restrict__ counts,
                                                  int* __restrict__ lists, int64_t stride) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int bin = -1;
  if (b < B) {
    const uint8_t* c = contact + b * 4 * N;
    int cnt = 0;
    if ((N & 3) == 0) {  // 4N bytes = N words
      const uint32_t* c4 = reinterpret_cast<const uint32_t*>(c);
      for (int i = 0; i < N; ++i) {
        const uint32_t v = c4[i];
        cnt += ((v & 0xffu) != 0) + ((v & 0xff00u) != 0) + ((v & 0xff0000u) != 0) +
               ((v >> 24) != 0);
      }
    } else {
      for (int i = 0; i < 4 * N; ++i) cnt += c[i] != 0;
    }
    const int nf = 3 * cnt;
    bin = kNumBins - 1;
    for (int q = 0; q < kNumBins; ++q)
      if (nf <= kBinCap[q]) { bin = q; break; }
  }
  // one atomic per (wave, bin)
#pragma unroll
  for (int q = 0; q < kNumBins; ++q) {
    const unsigned long long m = __ballot(bin == q);
    if (m == 0) continue;
    const int leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(&counts[q], __popcll(m));
    base = __shfl(base, leader, 64);
    if (bin == q) {
      const int rank = __popcll(m & ((1ull << lane) - 1ull));
      lists[(int64_t)q * stride + base + rank] = (int)b;
    }
  }
}

}  // namespace cmpc
