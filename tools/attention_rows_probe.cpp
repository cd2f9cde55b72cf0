// attention_rows_probe: at what rate does time attention's q | k | v buffer stream, fetched the way attention_time16_kernel
// fetches it and fetched as whole blocks?  (co-tracker_amd/csrc/attention.hip)
//
// A stand-alone replay of the memory traffic only: a qkv-shaped buffer of 103 424 token rows x 1152 floats (C3: 6464 tracks x 16
// frames; 476 MB, above the Infinity Cache) is read once per launch and 384 floats per row (159 MB) are written.
//   a  today's pattern: a WAVE owns a (track pair, head) job and reads, for each of q, k and v, the head's 192-byte slice of 32
//      rows as 6 loads of 16 bytes per lane (load i of lane l = chunk (64 i + l) % 12 of row (64 i + l) / 12); jobs head-fastest,
//      4 waves per workgroup, persistent walk with the stride of the grid.
//   b  the block pattern: a 512-thread WORKGROUP owns a track pair and reads its 147 456 contiguous bytes as 18 loads of 16 bytes
//      per lane, consecutive lanes consecutive 16 bytes (1 KiB per wave instruction); persistent walk.
//   t  as b with 256-thread workgroups that own ONE track (73 728 bytes): the same lines, half the bytes per workgroup.
// Every variant keeps 18 x 16 bytes per lane in flight: a lane sums its q, k and v chunks (the trivial consumer), issues the
// next job's loads into the same registers and stores the 6 sums while they fly -- the order of the product kernels, with no
// arithmetic to hide behind.  Knobs, all of them rows of the table: workgroups per CU and with them the bytes in flight per CU,
// and the cache policy of the loads (default | non-temporal: every byte is read once).
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/attention_rows_probe.cpp -o tools/attention_rows_probe
// Run:   tools/attention_rows_probe            (prints the table; every variant 3 warm-up + 10 timed launches, median)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define HIP_OK(x)                                                                           \
  do {                                                                                      \
    hipError_t e_ = (x);                                                                    \
    if (e_ != hipSuccess) {                                                                 \
      fprintf(stderr, "%s:%d %s -> %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));   \
      exit(2);                                                                              \
    }                                                                                       \
  } while (0)

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <bool NT>
__device__ __forceinline__ f32x4 ld16(const float* p) {
  if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
  else return *reinterpret_cast<const f32x4*>(p);
}

constexpr int TRACKS = 6464, FRAMES = 16, LD = 1152, HID = 384, HEADS = 8, HD = 48;
constexpr long ROWS = (long)TRACKS * FRAMES;  // 103 424
constexpr int PAIRS = TRACKS / 2;             // 3232

// a: one wave per (pair, head)
template <bool NT>
__global__ __launch_bounds__(256) void slices_kernel(const float* __restrict__ qkv, float* __restrict__ out, const long njobs) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long stride = (long)gridDim.x * 4;
  long job = (long)blockIdx.x * 4 + wave;
  if (job >= njobs) return;
  f32x4 raw[18];
  auto load = [&](const long jb) {
    const int head = (int)(jb % HEADS);
    const long row0 = (jb / HEADS) * 32;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int idx = 64 * i + lane, row = idx / 12, c = idx - 12 * row;
      const float* src = qkv + (row0 + row) * LD + head * HD + c * 4;
      raw[i] = ld16<NT>(src);
      raw[6 + i] = ld16<NT>(src + HID);
      raw[12 + i] = ld16<NT>(src + 2 * HID);
    }
  };
  load(job);
  while (true) {
    f32x4 acc[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[i] = raw[i] + raw[6 + i] + raw[12 + i];
    const long next = job + stride;
    const bool more = next < njobs;
    if (more) load(next);
    const int head = (int)(job % HEADS);
    const long row0 = (job / HEADS) * 32;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int idx = 64 * i + lane, row = idx / 12, c = idx - 12 * row;
      *reinterpret_cast<f32x4*>(out + (row0 + row) * HID + head * HD + c * 4) = acc[i];
    }
    if (!more) break;
    job = next;
  }
}

// b (THREADS = 512, a pair per workgroup) and t (THREADS = 256, a track per workgroup): 18 contiguous loads per lane
template <int THREADS, bool NT>
__global__ __launch_bounds__(THREADS) void blocks_kernel(const float* __restrict__ qkv, float* __restrict__ out, const int nblocks) {
  constexpr long IN = (long)THREADS * 18 * 4;  // floats per block: 36 864 (pair) | 18 432 (track)
  constexpr long OUT = IN / 3;
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  if (b >= nblocks) return;
  f32x4 raw[18];
  auto load = [&](const int bl) {
    const float* src = qkv + bl * IN + tid * 4;
#pragma unroll
    for (int i = 0; i < 18; ++i) raw[i] = ld16<NT>(src + i * THREADS * 4);
  };
  load(b);
  while (true) {
    f32x4 acc[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[i] = raw[i] + raw[6 + i] + raw[12 + i];
    const int next = b + (int)gridDim.x;
    const bool more = next < nblocks;
    if (more) load(next);
    float* dst = out + b * OUT + tid * 4;
#pragma unroll
    for (int i = 0; i < 6; ++i) *reinterpret_cast<f32x4*>(dst + i * THREADS * 4) = acc[i];
    if (!more) break;
    b = next;
  }
}

int main() {
  int dev = 0, cus = 0;
  HIP_OK(hipGetDevice(&dev));
  HIP_OK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const size_t in_bytes = (size_t)ROWS * LD * 4, out_bytes = (size_t)ROWS * HID * 4;
  float *qkv = nullptr, *out = nullptr;
  HIP_OK(hipMalloc(&qkv, in_bytes));
  HIP_OK(hipMalloc(&out, out_bytes));
  {
    std::vector<float> h((size_t)ROWS * LD);
    unsigned x = 12345u;
    for (auto& v : h) {
      x = x * 1664525u + 1013904223u;
      v = (float)(x >> 8) * (1.0f / 16777216.0f) - 0.5f;
    }
    HIP_OK(hipMemcpy(qkv, h.data(), in_bytes, hipMemcpyHostToDevice));
  }
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0));
  HIP_OK(hipEventCreate(&e1));
  printf("# attention_rows_probe: %ld rows x %d floats read (%.0f MB), %d floats per row written (%.0f MB); %d CUs\n", ROWS, LD, in_bytes / 1e6,
         HID, out_bytes / 1e6, cus);
  printf("# %-34s %5s %7s %12s %10s %10s %9s\n", "pattern", "loads", "WG/CU", "KiB fly/CU", "median us", "min us", "TB/s");
  struct Variant { char kind; int wgs; };
  const Variant variants[] = {{'a', 1}, {'a', 2}, {'a', 4}, {'b', 1}, {'b', 2}, {'t', 1}, {'t', 2}, {'t', 4}};
  for (int nt = 0; nt < 2; ++nt)
  for (const Variant& v : variants) {
    const int threads = v.kind == 'b' ? 512 : 256;
    const long units = v.kind == 'a' ? (long)PAIRS * HEADS / 4 : v.kind == 'b' ? PAIRS : TRACKS;  // workgroups' worth of work
    const unsigned grid = (unsigned)std::min<long>(units, (long)cus * v.wgs);
    auto launch = [&] {
      if (v.kind == 'a' && !nt) hipLaunchKernelGGL(slices_kernel<false>, dim3(grid), dim3(256), 0, 0, qkv, out, (long)PAIRS * HEADS);
      else if (v.kind == 'a') hipLaunchKernelGGL(slices_kernel<true>, dim3(grid), dim3(256), 0, 0, qkv, out, (long)PAIRS * HEADS);
      else if (v.kind == 'b' && !nt) hipLaunchKernelGGL((blocks_kernel<512, false>), dim3(grid), dim3(512), 0, 0, qkv, out, PAIRS);
      else if (v.kind == 'b') hipLaunchKernelGGL((blocks_kernel<512, true>), dim3(grid), dim3(512), 0, 0, qkv, out, PAIRS);
      else if (!nt) hipLaunchKernelGGL((blocks_kernel<256, false>), dim3(grid), dim3(256), 0, 0, qkv, out, TRACKS);
      else hipLaunchKernelGGL((blocks_kernel<256, true>), dim3(grid), dim3(256), 0, 0, qkv, out, TRACKS);
      HIP_OK(hipGetLastError());
    };
    for (int i = 0; i < 3; ++i) launch();
    HIP_OK(hipDeviceSynchronize());
    std::vector<float> us;
    for (int i = 0; i < 10; ++i) {
      HIP_OK(hipEventRecord(e0, 0));
      launch();
      HIP_OK(hipEventRecord(e1, 0));
      HIP_OK(hipEventSynchronize(e1));
      float ms = 0.0f;
      HIP_OK(hipEventElapsedTime(&ms, e0, e1));
      us.push_back(ms * 1000.0f);
    }
    std::sort(us.begin(), us.end());
    const double med = 0.5 * (us[4] + us[5]);
    const char* name = v.kind == 'a' ? "a head slices, wave per (pair,head)" : v.kind == 'b' ? "b pair block, 512 threads" : "t track block, 256 threads";
    printf("  %-34s %5s %7d %12d %10.1f %10.1f %9.2f\n", name, nt ? "nt" : "deflt", v.wgs, threads * 18 * 16 / 1024 * v.wgs, med, us[0], (in_bytes + out_bytes) / med * 1e-6);
  }
  {  // (the sums are read back once, so that the stores are visibly real)
    std::vector<float> h(1024);
    HIP_OK(hipMemcpy(h.data(), out, h.size() * 4, hipMemcpyDeviceToHost));
    double s = 0.0;
    for (float x : h) s += x;
    printf("# checksum of the first 1024 outputs of the last variant: %.6f\n", s);
  }
  HIP_OK(hipFree(qkv));
  HIP_OK(hipFree(out));
  return 0;
}
