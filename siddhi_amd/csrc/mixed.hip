// mixed.hip -- device side of an interleaved push (sdh_engine_push_mixed, native path)
// beside the MIX = true kernels of nfa_chain.hip: the pre-pass over `order`, and the event store's
// append of the parts' rows at their merged positions.
//
// Pre-pass: merged event k is the i-th occurrence of part p = order[k], i.e. event i of part p. A
// per-part exclusive scan of (order[k] == p) gives i: count per 256-event block (mix_count_kernel),
// scan the block counts per part (mix_scan_kernel, one wave per part), and write (mix_write_kernel)
// idx[k] = i, the merged ts[k] = ts_p[i] and the inverse map pos[pos_off[p] + i] = k. The host checks
// the totals against the parts' lengths between the scan and the write, so the write dereferences no
// index past a part (and guards it besides).
#include <hip/hip_runtime.h>

#include "launchers.h"
#include "nfa_types.h"

namespace sdh {
namespace {

constexpr int MIX_BLOCK = 256;

__device__ __forceinline__ int mix_mbcnt(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__global__ __launch_bounds__(MIX_BLOCK) void mix_count_kernel(MixPre A) {
  __shared__ int cnt[MIX_BLOCK / WAVE][MIX_MAXP];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * MIX_BLOCK + threadIdx.x;
  const int p = k < A.n ? A.order[k] : -1;
  if (k < A.n && (p < 0 || p >= A.n_parts)) atomicOr(&A.err[0], 1);
#pragma unroll
  for (int q = 0; q < MIX_MAXP; ++q) {
    const uint64_t m = __ballot(p == q);
    if (lane == 0) cnt[wv][q] = __popcll(m);
  }
  __syncthreads();
  if (threadIdx.x < MIX_MAXP) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < MIX_BLOCK / WAVE; ++w) c += cnt[w][threadIdx.x];
    A.blk_cnt[(int64_t)blockIdx.x * MIX_MAXP + threadIdx.x] = c;
  }
}

// blk_cnt[b][p] -> its exclusive scan over b, in place; total[p] = the sum. One wave per part.
__global__ __launch_bounds__(MIX_MAXP* WAVE) void mix_scan_kernel(MixPre A, int64_t n_blocks) {
  const int p = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int64_t carry = 0;
  for (int64_t b0 = 0; b0 < n_blocks; b0 += WAVE) {
    const int64_t b = b0 + lane;
    const int v = b < n_blocks ? A.blk_cnt[b * MIX_MAXP + p] : 0;
    int inc = v;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const int u = __shfl_up(inc, d, WAVE);
      if (lane >= d) inc += u;
    }
    // (a part longer than 2^31 - 1 events fails the host's length check: the clamp keeps idx an int)
    const int64_t ex = carry + inc - v;
    if (b < n_blocks) A.blk_cnt[b * MIX_MAXP + p] = (int)(ex < INT32_MAX ? ex : INT32_MAX);
    carry += __shfl(inc, WAVE - 1, WAVE);
  }
  if (lane == 0) A.total[p] = carry;
}

__global__ __launch_bounds__(MIX_BLOCK) void mix_write_kernel(MixPre A) {
  __shared__ int cnt[MIX_BLOCK / WAVE][MIX_MAXP];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * MIX_BLOCK + threadIdx.x;
  const int p = k < A.n ? A.order[k] : -1;
  int rank = 0;
#pragma unroll
  for (int q = 0; q < MIX_MAXP; ++q) {
    const uint64_t m = __ballot(p == q);
    if (lane == 0) cnt[wv][q] = __popcll(m);
    if (p == q) rank = mix_mbcnt(m);
  }
  __syncthreads();
  if (p < 0 || p >= A.n_parts) return;
  int before = 0;
  for (int w = 0; w < wv; ++w) before += cnt[w][p];
  const int64_t i = (int64_t)A.blk_cnt[(int64_t)blockIdx.x * MIX_MAXP + p] + before + rank;
  A.idx[k] = (int32_t)i;
  if (i < A.part_n[p]) {
    A.ts_out[k] = A.ts[p][i];
    A.pos[A.pos_off[p] + i] = (int32_t)k;
  } else {
    A.ts_out[k] = 0;
  }
}

// the event store (select.hip store_append_kernel) for one part of an interleaved push: row of event i
// at merged position pos[i]; the events whose merged position is before `first` are not kept (a call
// longer than the ring keeps its last ev_cap merged events)
__global__ __launch_bounds__(256) void store_append_mixed_kernel(StreamBatch B, uint32_t float_mask,
                                                                 const int32_t* __restrict__ pos, int64_t first,
                                                                 int64_t* __restrict__ rows, int64_t mask, int W) {
  const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= B.n * W) return;
  const int64_t i = x / W;
  const int w = (int)(x - i * W);
  const int64_t k = pos[i];
  if (k < first) return;
  int64_t v = 0;
  if (w == 0) {
    v = B.ts[i];
  } else if (w == 1) {
#pragma unroll
    for (int a = 0; a < MAXATTR; ++a)
      if (a < B.n_attr && B.nul[a] && B.nul[a][i]) v |= (int64_t)1 << a;
  } else {
#pragma unroll
    for (int a = 0; a < MAXATTR; ++a) {
      if (a != w - 2 || a >= B.n_attr) continue;
      if (B.width[a] == 8) v = static_cast<const int64_t*>(B.col[a])[i];
      else if (B.width[a] == 1) v = static_cast<const uint8_t*>(B.col[a])[i];
      else if ((float_mask >> a) & 1u) v = (int64_t)static_cast<const uint32_t*>(B.col[a])[i];
      else v = (int64_t)static_cast<const int32_t*>(B.col[a])[i];
    }
  }
  rows[((B.seq_base + k) & mask) * W + w] = v;
}

}  // namespace
}  // namespace sdh

extern "C" int64_t sdh_mix_blocks(int64_t n) { return (n + sdh::MIX_BLOCK - 1) / sdh::MIX_BLOCK; }

// count + scan: blk_cnt scanned, total[] and err[0] set (the host reads them before the write)
extern "C" hipError_t sdh_mix_count(const sdh::MixPre* A, hipStream_t s) {
  if (A->n <= 0) return hipSuccess;
  const int64_t nb = sdh_mix_blocks(A->n);
  hipLaunchKernelGGL(sdh::mix_count_kernel, dim3((unsigned)nb), dim3(sdh::MIX_BLOCK), 0, s, *A);
  hipLaunchKernelGGL(sdh::mix_scan_kernel, dim3(1), dim3(sdh::MIX_MAXP * sdh::WAVE), 0, s, *A, nb);
  return hipGetLastError();
}

extern "C" hipError_t sdh_mix_write(const sdh::MixPre* A, hipStream_t s) {
  if (A->n <= 0) return hipSuccess;
  hipLaunchKernelGGL(sdh::mix_write_kernel, dim3((unsigned)sdh_mix_blocks(A->n)), dim3(sdh::MIX_BLOCK), 0, s, *A);
  return hipGetLastError();
}

extern "C" hipError_t sdh_store_append_mixed(const sdh::StreamBatch* B, uint32_t float_mask, const int32_t* pos,
                                             int64_t first, int64_t* rows, int64_t mask, int W, hipStream_t s) {
  if (B->n <= 0) return hipSuccess;
  const int64_t n = B->n * W;
  hipLaunchKernelGGL(sdh::store_append_mixed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, *B, float_mask,
                     pos, first, rows, mask, W);
  return hipGetLastError();
}
