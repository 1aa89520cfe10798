// calib.hip -- the HBM ceiling the roofline fractions are also reported against (bench.py
// roofline.measured): a streaming copy (read + write, the shape of the NFA kernels' traffic) and a
// streaming read over buffers far larger than the 256 MB MALL, 16-B vector accesses, grid-stride over
// 8 or 32 workgroups of 256 per CU (or one element per thread), several launches timed with HIP
// events, the best kept.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

__global__ __launch_bounds__(256) void copy_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n; i += 4 * stride) {
    const uint4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
    dst[i] = a;
    dst[i + stride] = b;
    dst[i + 2 * stride] = c;
    dst[i + 3 * stride] = d;
  }
  for (; i < n; i += stride) dst[i] = src[i];
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(256) void copy1_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src) + i);
    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(dst) + i);
  }
}

__global__ __launch_bounds__(256) void read_kernel(const uint4* __restrict__ src, int64_t n, uint32_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t acc = 0;
  for (; i + 3 * stride < n; i += 4 * stride) {
    const uint4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
    acc ^= a.x ^ a.y ^ a.z ^ a.w ^ b.x ^ b.y ^ b.z ^ b.w ^ c.x ^ c.y ^ c.z ^ c.w ^ d.x ^ d.y ^ d.z ^ d.w;
  }
  for (; i < n; i += stride) acc ^= src[i].x ^ src[i].y ^ src[i].z ^ src[i].w;
  if (acc == 0x9E3779B9u) out[0] = acc;  // (keeps the loads; practically never stores)
}

// ---- the write-stream probe (sdh_calibrate_store) ----
// linear fill: 16 B per lane, grid-stride, nothing read
template <bool NT>
__global__ __launch_bounds__(256) void fill_kernel(u32x4* __restrict__ dst, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const u32x4 v = {(uint32_t)i, 1u, 2u, 3u};
  for (; i < n; i += stride) {
    if (NT) __builtin_nontemporal_store(v, dst + i);
    else dst[i] = v;
  }
}

struct StoreProbe {
  char* buf;
  int32_t* next;     // [0] the next free block
  int32_t n_blocks;  // blocks of block_bytes in buf
  int32_t block_bytes, burst_bytes;
  int32_t side;   // side entries per block: > 0 as 8-B single-lane stores between the bursts, < 0 whole at block close
  int32_t claim;  // 0: the claim behind the last burst, 1: one block ahead
  int32_t ragged;
};

// Block pattern: K_ratchet's emission store stream with nothing else (nfa_ratchet_shared.hip). One wave
// per workgroup with the 8-KiB window, blocks claimed from a counter, each filled upwards in bursts of
// ds_read_b128 + 1-KiB buffer stores through a descriptor of the block, side entries walking down from
// the block's end. Every store goes through the block's descriptor, whose size bounds it.
template <int AUX>
__global__ __launch_bounds__(64) void block_store_kernel(StoreProbe P) {
  __shared__ __attribute__((aligned(16))) uint32_t win[2048];
  const int lane = threadIdx.x;
  for (int i = lane; i < 2048; i += 64) win[i] = (uint32_t)i;
  __syncthreads();
  auto claim = [&]() {
    int nb = 0;
    // (a wrapping increment, not atomicAdd: the compiler's wave reduction of a uniform add reads the
    // result, and waits for it, right behind the atomic)
    if (lane == 0) nb = (int)atomicInc(reinterpret_cast<unsigned int*>(P.next), 0xffffffffu);
    return nb;  // (lane 0's; read through readfirstlane where it is used)
  };
  const int cap = P.block_bytes;
  const int ns = P.side < 0 ? -P.side : P.side;
  const int payload = (cap - 8 * ns) & ~15;
  const int n_bursts = (payload + P.burst_bytes - 1) / P.burst_bytes;
  int cur = claim();
  int ahead = P.claim ? claim() : 0;
  for (uint32_t round = 0;; ++round) {
    const int nb = __builtin_amdgcn_readfirstlane(cur);
    if (nb >= P.n_blocks) break;
    const uint64_t base = (uint64_t)(P.buf + (size_t)nb * cap);
    const uint32_t blo = __builtin_amdgcn_readfirstlane((uint32_t)base), bhi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)bhi << 32) | blo), 0, cap, 0x00020000);
    int nxt = 0;
    if (P.claim) {  // the block after the next, claimed now and first read a whole block later
      nxt = claim();
    }
    int sdone = 0;
    for (int k = 0; k < n_bursts; ++k) {
      win[lane] = round + (uint32_t)k;  // (the scatter's stand-in: the window changes between bursts)
      __syncthreads();
      const int b0 = k * P.burst_bytes, b1 = min(b0 + P.burst_bytes, payload);
      int q0 = b0, q1 = b1;
      if (P.ragged && b1 - b0 >= 32) {  // three dwords at either end, as a pass whose fill & 3 is 1
        q0 = b0 + 16;
        q1 = b1 - 16;
        if (lane < 6) {
          const int o = lane < 3 ? b0 + 4 + 4 * lane : q1 + 4 * (lane - 3);
          __builtin_amdgcn_raw_buffer_store_b32(win[lane], rs, o, 0, AUX);
        }
      }
      for (int o = q0 + 16 * lane; o < q1; o += 1024) {
        const u32x4 v = reinterpret_cast<const u32x4*>(win)[(o & 8191) >> 4];
        __builtin_amdgcn_raw_buffer_store_b128(v, rs, o, 0, AUX);
      }
      __syncthreads();
      if (P.side > 0) {
        const int upto = (int)((int64_t)ns * (k + 1) / n_bursts);
        for (; sdone < upto; ++sdone)
          if (lane == 0) {
            const u32x2 se = {(uint32_t)sdone, round};
            __builtin_amdgcn_raw_buffer_store_b64(se, rs, cap - 8 * (sdone + 1), 0, 0);
          }
      }
    }
    if (P.side < 0) {  // the side entries whole, 16 B per lane
      const int s0 = (cap - 8 * ns) & ~15;
      for (int o = s0 + 16 * lane; o < cap; o += 1024) {
        const u32x4 v = reinterpret_cast<const u32x4*>(win)[(o & 8191) >> 4];
        __builtin_amdgcn_raw_buffer_store_b128(v, rs, o, 0, AUX);
      }
    }
    if (P.claim) {
      // (the claimed index passes through here and no earlier: left to itself the compiler reads it,
      // and waits for it, right behind the atomic)
      asm volatile("" : "+v"(ahead));
      cur = ahead;
      ahead = nxt;
    } else {
      cur = claim();
    }
  }
}

}  // namespace

// The write-only rate of `device` over a `bytes`-sized buffer, best of `iters` (GB/s of bytes stored).
// mode 0: linear fill, params = {nt}. mode 1: the block pattern, params = {side, claim, nt, block KiB,
// burst KiB, ragged} (StoreProbe). The probe writes into its own allocation only.
extern "C" int sdh_calibrate_store(int32_t device, int64_t bytes, int32_t iters, int32_t mode, const int32_t* params,
                                   double* out_gbps) {
  if (bytes < (1 << 20) || iters < 1 || !params || !out_gbps || (mode != 0 && mode != 1)) return -1;
  const int nt = mode == 0 ? params[0] : params[2];
  const int side = mode ? params[0] : 0, claim = mode ? params[1] : 0;
  const int block_kib = mode ? params[3] : 64, burst_kib = mode ? params[4] : 8, ragged = mode ? params[5] : 0;
  if (nt != 0 && nt != 1) return -1;
  if (mode == 1) {
    if ((block_kib != 16 && block_kib != 64 && block_kib != 256) || (burst_kib != 4 && burst_kib != 8 && burst_kib != 16) ||
        (claim != 0 && claim != 1) || (ragged != 0 && ragged != 1) || side < -1024 || side > 1024)
      return -1;
  }
  if (hipSetDevice(device) != hipSuccess) return -3;
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  char* buf = nullptr;
  int32_t* next = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipStream_t s = nullptr;
  int rc = 0;
  if (hipMalloc(&buf, (size_t)bytes) != hipSuccess || hipMalloc(&next, 4) != hipSuccess || hipEventCreate(&e0) != hipSuccess ||
      hipEventCreate(&e1) != hipSuccess || hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
    rc = -3;
  } else {
    StoreProbe P;
    P.buf = buf;
    P.next = next;
    P.block_bytes = block_kib << 10;
    P.burst_bytes = burst_kib << 10;
    P.n_blocks = mode == 1 ? (int32_t)(bytes / P.block_bytes) : 0;
    P.side = side;
    P.claim = claim;
    P.ragged = ragged;
    const int64_t n16 = bytes / 16;
    double stored = (double)n16 * 16;
    if (mode == 1) {
      const int ns = side < 0 ? -side : side;
      const int payload = (P.block_bytes - 8 * ns) & ~15;
      const int n_bursts = (payload + P.burst_bytes - 1) / P.burst_bytes;
      double per = payload + 8.0 * ns;
      if (ragged) per -= 8.0 * n_bursts;  // (of each burst's end quads, three dwords are written)
      stored = per * P.n_blocks;
    }
    float best = 1e30f;
    for (int it = 0; it < iters + 1; ++it) {  // (the first round warms up)
      for (int per_cu : {8, 32}) {
        if (mode == 1 && per_cu != 8) continue;
        (void)hipMemsetAsync(next, 0, 4, s);
        (void)hipEventRecord(e0, s);
        if (mode == 0) {
          const dim3 grid(cus * per_cu), block(256);
          if (nt) hipLaunchKernelGGL(fill_kernel<true>, grid, block, 0, s, reinterpret_cast<u32x4*>(buf), n16);
          else hipLaunchKernelGGL(fill_kernel<false>, grid, block, 0, s, reinterpret_cast<u32x4*>(buf), n16);
        } else {
          // more workgroups than are resident (the 8-KiB window holds 20 waves on a CU): the hardware
          // keeps every slot filled, as in the emission kernel's launch
          const dim3 grid(cus * 40), block(64);
          if (nt) hipLaunchKernelGGL(block_store_kernel<2>, grid, block, 0, s, P);
          else hipLaunchKernelGGL(block_store_kernel<0>, grid, block, 0, s, P);
        }
        (void)hipEventRecord(e1, s);
        (void)hipEventSynchronize(e1);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        if (it && ms < best) best = ms;
      }
    }
    if (hipGetLastError() != hipSuccess) rc = -3;
    *out_gbps = stored / (best * 1e-3) / 1e9;
  }
  if (s) (void)hipStreamSynchronize(s);
  if (buf) (void)hipFree(buf);
  if (next) (void)hipFree(next);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (s) (void)hipStreamDestroy(s);
  return rc;
}

// Best-of-`iters` streaming copy and read bandwidth (GB/s of bytes moved: copy counts read + write)
// over `bytes`-sized buffers on `device`.
extern "C" int sdh_calibrate_hbm(int32_t device, int64_t bytes, int32_t iters, double* copy_gbps, double* read_gbps) {
  if (bytes < (1 << 20) || iters < 1 || !copy_gbps || !read_gbps) return -1;
  if (hipSetDevice(device) != hipSuccess) return -3;
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  const int64_t n = bytes / 16;
  uint4 *a = nullptr, *b = nullptr;
  uint32_t* o = nullptr;
  int rc = 0;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipStream_t s = nullptr;
  if (hipMalloc(&a, n * 16) != hipSuccess || hipMalloc(&b, n * 16) != hipSuccess || hipMalloc(&o, 4) != hipSuccess ||
      hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess ||
      hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
    rc = -3;
  } else {
    (void)hipMemsetAsync(a, 1, n * 16, s);
    (void)hipMemsetAsync(b, 0, n * 16, s);
    const dim3 block(256);
    float best_c = 1e30f, best_r = 1e30f;
    auto timed = [&](auto launch) {
      float ms = 0;
      (void)hipEventRecord(e0, s);
      launch();
      (void)hipEventRecord(e1, s);
      (void)hipEventSynchronize(e1);
      (void)hipEventElapsedTime(&ms, e0, e1);
      return ms;
    };
    // grid-stride at 8 / 32 workgroups per CU, and one element per thread with nontemporal stores:
    // the best of them is the ceiling
    for (int it = 0; it < iters + 1; ++it) {  // (the first round warms up)
      for (int per_cu : {8, 32}) {
        const dim3 grid(cus * per_cu);
        const float c = timed([&] { hipLaunchKernelGGL(copy_kernel, grid, block, 0, s, a, b, n); });
        const float r = timed([&] { hipLaunchKernelGGL(read_kernel, grid, block, 0, s, a, n, o); });
        if (it) {
          best_c = c < best_c ? c : best_c;
          best_r = r < best_r ? r : best_r;
        }
      }
      const dim3 g1((unsigned)((n + 255) / 256));
      const float c1 = timed([&] { hipLaunchKernelGGL(copy1_kernel, g1, block, 0, s, a, b, n); });
      if (it) best_c = c1 < best_c ? c1 : best_c;
    }
    if (hipGetLastError() != hipSuccess) rc = -3;
    *copy_gbps = 2.0 * (double)n * 16 / (best_c * 1e-3) / 1e9;
    *read_gbps = (double)n * 16 / (best_r * 1e-3) / 1e9;
  }
  if (s) (void)hipStreamSynchronize(s);
  if (a) (void)hipFree(a);
  if (b) (void)hipFree(b);
  if (o) (void)hipFree(o);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (s) (void)hipStreamDestroy(s);
  return rc;
}
