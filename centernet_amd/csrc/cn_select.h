// cn_select.h -- the exact select every decode kernel shares (cn_decode.hip, cn_decode_tasks.hip): the 64-bit
// (score, ~index) keys, radix_select over a histogram in LDS, collect_and_sort (a one-wave bitonic network),
// and the rounding rule of the decode files.  Include it FIRST among the file's own code: the pragma below is
// file-scope and holds from here to the end of the translation unit.
#pragma once
#include "cn_common.h"

// Decode arithmetic must round exactly like the reference's torch ops (bit-exact parity):
// no mul+add fusion anywhere in a file that includes this one (hipcc's default is
// -ffp-contract=fast-honor-pragmas and HIP's __fmul_rn/__fadd_rn are plain operators).
#pragma clang fp contract(off)
// Rounded-once helpers compiled under contract(off): unlike HIP's header-inline __fmul_rn /
// __fadd_rn their results can never be fused into an FMA after inlining.
static __device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
static __device__ __forceinline__ float add_rn(float a, float b) { return a + b; }

namespace {

constexpr int NT = 256;      // threads per workgroup (4 waves)
constexpr int KMAX = 128;    // largest supported K
constexpr int HBINS = 2048;  // radix-select histogram bins (11-bit digits)

typedef unsigned long long u64;
constexpr int NTM = 1024;  // threads of the one-workgroup-per-image kernels (merge, exct select)

// Order-preserving float -> uint32 map (larger float -> larger key).
__device__ __forceinline__ uint32_t f2key(float v)
{
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k)
{
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __uint_as_float(u);
}
constexpr uint32_t KEY_ZERO = 0x80000000u;  // f2key(+0.0f)

constexpr int MAXW = 16;  // waves of the largest workgroup that uses SelShared (1024 threads)

struct SelShared {
    uint32_t hist[HBINS];
    u64 sel[KMAX];
    uint32_t wsum[MAXW];
    uint32_t cnt;
    uint32_t digit, need, bincount;
    uint32_t ncand;
    uint32_t pad_[3];
};
static_assert(sizeof(SelShared) % 16 == 0, "keep the LDS carve 16-byte aligned");

__device__ __forceinline__ int pass_shift(int p)
{
    // 64-bit key split into digits of 11,11,10 | 11,11,10 bits (msb first)
    return p == 0 ? 53 : p == 1 ? 42 : p == 2 ? 32 : p == 3 ? 21 : p == 4 ? 10 : 0;
}
__device__ __forceinline__ uint32_t pass_dmask(int p) { return (p == 2 || p == 5) ? 1023u : 2047u; }

// The bin of sh.hist that holds the `need`-th largest element, counted from the top bin down: on return (behind
// a barrier) sh.digit is that bin, sh.need what is still needed from inside it and sh.bincount its population.
// Called by all TB threads with sh.hist complete and a barrier behind its last update.
template <int TB>
__device__ __forceinline__ void pick_bin(SelShared &sh, uint32_t need)
{
    static_assert(HBINS % TB == 0 && TB / CN_WAVE <= MAXW, "block size");
    constexpr int BPT = HBINS / TB;  // histogram bins owned by a thread
    const int tid = threadIdx.x;
    const int lane = tid & (CN_WAVE - 1);
    const int wave = tid / CN_WAVE;
    // suffix sums over bins: thread t owns bins [BPT*t, BPT*t + BPT)
    uint32_t p = 0;
#pragma unroll
    for (int j = 0; j < BPT; ++j) p += sh.hist[tid * BPT + j];
    uint32_t s = p;
#pragma unroll
    for (int o = 1; o < CN_WAVE; o <<= 1) {
        const uint32_t t = __shfl_down(s, o);
        if (lane + o < CN_WAVE) s += t;
    }
    if (lane == 0) sh.wsum[wave] = s;
    __syncthreads();
    for (int w = wave + 1; w < TB / CN_WAVE; ++w) s += sh.wsum[w];
    const uint32_t above = s - p;  // elements in strictly higher bins
    if (above < need && s >= need) {
        uint32_t run = above;
        for (int j = BPT - 1; j >= 0; --j) {
            const uint32_t h = sh.hist[tid * BPT + j];
            if (run + h >= need) {
                sh.digit = tid * BPT + j;
                sh.need = need - run;
                sh.bincount = h;
                break;
            }
            run += h;
        }
    }
    __syncthreads();
}

// Exact selection of the `need0` largest 64-bit keys among the elements that
// `for_each(f)` enumerates (f(key64, is_plain_zero)); keys must be distinct.
// On return every thread holds (prefix, mask): an element is selected iff
// (key & mask) >= prefix.  Elements whose score is exactly +0.0 (the ~89 % of a
// heat-map that the peak test suppressed) are counted per wave instead of one
// LDS atomic each, otherwise they would serialise on a single histogram bin.
template <int TB, class ForEach>
__device__ __forceinline__ void radix_select(ForEach &&for_each, uint32_t need0, SelShared &sh,
                                             u64 &out_prefix, u64 &out_mask)
{
    static_assert(HBINS % TB == 0 && TB / CN_WAVE <= MAXW, "block size");
    const int tid = threadIdx.x;
    const int lane = tid & (CN_WAVE - 1);
    u64 prefix = 0, mask = 0;
    uint32_t need = need0;
    const u64 zkey = (u64)KEY_ZERO << 32;
#pragma unroll 1
    for (int pass = 0; pass < 6; ++pass) {
        const int shift = pass_shift(pass);
        const uint32_t dmask = pass_dmask(pass);
        for (int i = tid; i < HBINS; i += TB) sh.hist[i] = 0;
        __syncthreads();
        uint32_t zc = 0;
        for_each([&](u64 k, bool plain_zero) {
            if ((k & mask) == prefix) {
                if (plain_zero && pass < 3)
                    ++zc;
                else
                    atomicAdd(&sh.hist[(uint32_t)(k >> shift) & dmask], 1u);
            }
        });
        if (pass < 3) {
            for (int o = CN_WAVE / 2; o > 0; o >>= 1) zc += __shfl_down(zc, o);
            if (lane == 0 && zc) atomicAdd(&sh.hist[(uint32_t)(zkey >> shift) & dmask], zc);
        }
        __syncthreads();
        pick_bin<TB>(sh, need);
        prefix |= (u64)sh.digit << shift;
        mask |= (u64)dmask << shift;
        need = sh.need;
        if (sh.bincount == need) break;  // the whole bin is taken: done
    }
    out_prefix = prefix;
    out_mask = mask;
}

// Collect the selected keys into sh.sel[0..KMAX) and sort them descending.  The sort is a
// 128-element bitonic network run by ONE wave (two keys per lane, cross-lane exchange by
// shuffles): no workgroup barriers inside the network.
template <int TB, class ForEach>
__device__ __forceinline__ void collect_and_sort(ForEach &&for_each, u64 prefix, u64 mask,
                                                 SelShared &sh)
{
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid == 0) sh.cnt = 0;
    for (int i = tid; i < KMAX; i += TB) sh.sel[i] = 0;  // pad keys sort last
    __syncthreads();
    for_each([&](u64 k, bool) {
        if ((k & mask) >= prefix) {
            const uint32_t pos = atomicAdd(&sh.cnt, 1u);
            if (pos < (uint32_t)KMAX) sh.sel[pos] = k;
        }
    });
    __syncthreads();
    if (tid < CN_WAVE) {
        const int lane = tid;
        u64 v[2] = {sh.sel[lane], sh.sel[lane + CN_WAVE]};
        for (int k = 2; k <= KMAX; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                if (j == CN_WAVE) {  // partner = the lane's other slot (only when k == 128)
                    const u64 hi = v[0] > v[1] ? v[0] : v[1];
                    const u64 lo = v[0] > v[1] ? v[1] : v[0];
                    v[0] = hi;
                    v[1] = lo;
                } else {
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const int i = s * CN_WAVE + lane;
                        const uint32_t olo = __shfl_xor((uint32_t)v[s], j);
                        const uint32_t ohi = __shfl_xor((uint32_t)(v[s] >> 32), j);
                        const u64 o = ((u64)ohi << 32) | olo;
                        const bool desc = (i & k) == 0;
                        const bool lower = (i & j) == 0;
                        const bool take_max = (lower == desc);
                        v[s] = take_max ? (v[s] > o ? v[s] : o) : (v[s] > o ? o : v[s]);
                    }
                }
            }
        }
        sh.sel[lane] = v[0];
        sh.sel[lane + CN_WAVE] = v[1];
    }
    __syncthreads();
}

}  // namespace
