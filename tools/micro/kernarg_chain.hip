// Micro-benchmark: what a kernel pays for reading its arguments as a CHAIN of scalar loads (tools/micro is not part of the library).
// A conv kernel whose argument struct is ~1 KB reads it in several batches of s_load_dword*, each behind its own
// `s_waitcnt lgkmcnt(0)`: dependent scalar round trips before the first operand load can issue (profiles/conv_prologue.md).
// The kernel below takes a 1 KB by-value struct and reads N of its 64-byte lines either as N data-dependent scalar loads (each
// address comes out of the previous load) or as ONE batch of N independent loads behind one wait, first with the lines cold (a
// launch starts with an invalidated scalar cache, and every launch gets a fresh argument buffer), then again warm.  Launches are
// back to back with fresh argument values.  Reported: s_memtime ticks and ns per dependent round trip, cold and warm, and the cost
// of the single batch.
// Build: hipcc --offload-arch=gfx950 -O3 kernarg_chain.hip -o kernarg_chain
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>

struct Big { unsigned v[256]; };        // v[32 l]: byte offset of the next line of the chain; v[254..255]: the result pointer

// one dependent hop: off = *(unsigned*)(kernarg + off)
#define HOP(off, kp) asm volatile("s_load_dword %0, %1, %0\n\ts_waitcnt lgkmcnt(0)" : "+s"(off) : "s"(kp) : "memory")

template <int N, bool BATCH>
__global__ __launch_bounds__(64) void chain(const Big) {
    const long long t0 = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_sched_barrier(0);
    const auto kp = __builtin_amdgcn_kernarg_segment_ptr();      // (constant address space: a 64-bit SGPR pair)
    unsigned sum = 0;
    long long t1, t2;
    if constexpr (BATCH) {
        static_assert(N == 8, "the batch variant is written for eight lines");
        unsigned a0, a1, a2, a3, a4, a5, a6, a7;
#define BATCH8() asm volatile("s_load_dword %0, %8, 0x0\n\ts_load_dword %1, %8, 0x80\n\ts_load_dword %2, %8, 0x100\n\ts_load_dword %3, %8, 0x180\n\t" \
                              "s_load_dword %4, %8, 0x200\n\ts_load_dword %5, %8, 0x280\n\ts_load_dword %6, %8, 0x300\n\ts_load_dword %7, %8, 0x380\n\t" \
                              "s_waitcnt lgkmcnt(0)" : "=&s"(a0), "=&s"(a1), "=&s"(a2), "=&s"(a3), "=&s"(a4), "=&s"(a5), "=&s"(a6), "=&s"(a7) : "s"(kp) : "memory")
        BATCH8();
        sum += a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;
        asm volatile("" : "+s"(sum));
        t1 = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
        BATCH8();
        sum += a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;
        asm volatile("" : "+s"(sum));
        t2 = __builtin_amdgcn_s_memtime();
    } else {
        unsigned off = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) HOP(off, kp);
        sum += off;
        t1 = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
        off = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) HOP(off, kp);
        sum += off;
        t2 = __builtin_amdgcn_s_memtime();
    }
    __builtin_amdgcn_sched_barrier(0);
    unsigned long long res;
    asm volatile("s_load_dwordx2 %0, %1, 0x3f8\n\ts_waitcnt lgkmcnt(0)" : "=s"(res) : "s"(kp) : "memory");
    long long* out = reinterpret_cast<long long*>(res);
    if (threadIdx.x == 0) {
        out[blockIdx.x * 4 + 0] = t1 - t0;
        out[blockIdx.x * 4 + 1] = t2 - t1;
        out[blockIdx.x * 4 + 2] = (long long)sum;
    }
}

// s_memtime ticks per microsecond: both counters around a ~1 ms spin (s_memrealtime runs at 100 MHz)
__global__ void calib(long long* out) {
    const long long r0 = __builtin_amdgcn_s_memrealtime(), t0 = __builtin_amdgcn_s_memtime();
    long long r1 = r0;
    while (r1 - r0 < 100000) r1 = __builtin_amdgcn_s_memrealtime();
    const long long t1 = __builtin_amdgcn_s_memtime();
    out[0] = t1 - t0; out[1] = r1 - r0;
}

static double median(std::vector<long long>& v) {
    std::sort(v.begin(), v.end());
    return v.empty() ? 0.0 : (double)v[v.size() / 2];
}

template <int N, bool BATCH>
static void run(int blocks, int launches, double ns_per_tick) {
    long long* out;
    (void)hipMalloc(&out, (size_t)launches * blocks * 4 * sizeof(long long));
    (void)hipMemset(out, 0, (size_t)launches * blocks * 4 * sizeof(long long));
    for (int l = 0; l < launches; ++l) {
        Big a;
        for (int i = 0; i < 256; ++i) a.v[i] = 0x5a5a0000u + (unsigned)(l * 256 + i);      // fresh values every launch
        // the chain walks the eight 128-byte-spaced lines in an order that changes with the launch and ends on line 0
        int order[8];
        for (int i = 0; i < 8; ++i) order[i] = i == 0 ? 0 : 1 + (i - 1 + l) % 7;
        for (int i = 0; i < 8; ++i) a.v[order[i] * 32] = (unsigned)(order[(i + 1) % 8] * 128);
        const unsigned long long p = (unsigned long long)(out + (size_t)l * blocks * 4);
        a.v[254] = (unsigned)p; a.v[255] = (unsigned)(p >> 32);
        hipLaunchKernelGGL((chain<N, BATCH>), dim3(blocks), dim3(64), 0, 0, a);
    }
    (void)hipDeviceSynchronize();
    std::vector<long long> h((size_t)launches * blocks * 4);
    (void)hipMemcpy(h.data(), out, h.size() * sizeof(long long), hipMemcpyDeviceToHost);
    std::vector<long long> cold, warm, cold_first;
    for (int l = 2; l < launches; ++l)                      // (the first launches load the code object)
        for (int b = 0; b < blocks; ++b) {
            cold.push_back(h[((size_t)l * blocks + b) * 4]);
            warm.push_back(h[((size_t)l * blocks + b) * 4 + 1]);
            if (b == 0) cold_first.push_back(h[((size_t)l * blocks + b) * 4]);
        }
    const double c = median(cold), w = median(warm), cf = median(cold_first);
    const int trips = BATCH ? 1 : N;
    printf("%-22s blocks %4d: cold %7.0f ticks = %7.1f ns (%6.1f ns per round trip), first block %7.1f ns; warm %6.0f ticks = %6.1f ns (%5.1f ns per round trip)\n",
           BATCH ? "one batch of 8 loads" : (N == 8 ? "8 dependent loads" : N == 4 ? "4 dependent loads" : "1 load"), blocks, c, c * ns_per_tick,
           c * ns_per_tick / trips, cf * ns_per_tick, w, w * ns_per_tick, w * ns_per_tick / trips);
    (void)hipFree(out);
}

int main() {
    long long* cal;
    (void)hipMalloc(&cal, 16);
    hipLaunchKernelGGL(calib, dim3(1), dim3(1), 0, 0, cal);
    hipLaunchKernelGGL(calib, dim3(1), dim3(1), 0, 0, cal);
    long long hc[2];
    (void)hipMemcpy(hc, cal, 16, hipMemcpyDeviceToHost);
    const double ns_per_tick = (double)hc[1] * 10.0 / (double)hc[0];
    printf("s_memtime: %.4f ns per tick (%.1f MHz)\n", ns_per_tick, 1e3 / ns_per_tick);
    for (int blocks : {1, 296, 1184}) {
        run<1, false>(blocks, 60, ns_per_tick);
        run<4, false>(blocks, 60, ns_per_tick);
        run<8, false>(blocks, 60, ns_per_tick);
        run<8, true>(blocks, 60, ns_per_tick);
    }
    (void)hipFree(cal);
    return 0;
}
