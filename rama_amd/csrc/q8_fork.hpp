// q8_fork.hpp -- the FORK of cached KV rows (rama_q8_kv_fork): rows [0, n_rows) of every layer of one run
// state's key and value caches, copied into up to kForkMaxDst other run states.  Within one layer those rows are one contiguous
// span of n_rows * dim floats, so a fork is 2 * n_layers spans, each read ONCE and written n_dst times: (n_dst + 1) spans of
// traffic where n_dst device-to-device copies move 2 * n_dst.
//   one launch: grid = (pieces of a span, layer x {k, v}); a workgroup moves kForkPiece consecutive 16-byte words of its span
//   a thread issues its kForkLoads loads -- independent, unconditional, at addresses clamped into the span (DESIGN.md section 7:
//   `cond ? load : 0` is a branch with a full wait behind it) -- before its first store; what lies behind the span's end is
//   selected away at the stores
//   every access is a non-temporal one in the global address space (chain.hpp's gptr4): a 7B prefix of 1 000 rows is about 1 GB
//   that nobody reads again soon and that should not take the weights' cache lines
// A cache base that is not 16-byte aligned (a caller-owned run state uploaded tensor by tensor) takes kv_fork_kernel<false>: the same
// grid over 4-byte words, the same bytes written.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"

namespace rama {

constexpr int kForkMaxDst = 16;
constexpr int kForkThreads = 256;
constexpr int kForkLoads = 4;                                    // independent loads in flight per thread
constexpr int kForkPiece = kForkThreads * kForkLoads;            // words of a span per workgroup

struct ForkParams {
    const float* src[2];               // the source's key and value cache
    float* dst[2][kForkMaxDst];        // every destination's
    int n_dst;
    unsigned long long layer_floats;   // seq_len * dim: from one layer's rows to the next layer's
    unsigned long long n_words;        // words in a span (VEC: 16 bytes each; else 4 bytes each); >= 1
};

template <bool VEC> struct ForkWord;
template <> struct ForkWord<true> { typedef f4 type; };
template <> struct ForkWord<false> { typedef float type; };

template <bool VEC>
__global__ __launch_bounds__(kForkThreads) void kv_fork_kernel(ForkParams p) {
    typedef typename ForkWord<VEC>::type W;
    typedef const __attribute__((address_space(1))) W* gin;
    typedef __attribute__((address_space(1))) W* gout;
    const int kv = blockIdx.y & 1;
    const unsigned long long layer = blockIdx.y >> 1;
    const unsigned long long off = layer * p.layer_floats;         // floats from the cache base to the span
    const unsigned long long w0 = (unsigned long long)blockIdx.x * kForkPiece + threadIdx.x;
    const gin s = (gin)reinterpret_cast<const W*>(p.src[kv] + off);
    W v[kForkLoads];
#pragma unroll
    for (int u = 0; u < kForkLoads; u++) {
        const unsigned long long i = w0 + (unsigned long long)u * kForkThreads;
        v[u] = __builtin_nontemporal_load(s + (i < p.n_words ? i : p.n_words - 1));
    }
    for (int d = 0; d < p.n_dst; d++) {
        const gout o = (gout)reinterpret_cast<W*>(p.dst[kv][d] + off);
#pragma unroll
        for (int u = 0; u < kForkLoads; u++) {
            const unsigned long long i = w0 + (unsigned long long)u * kForkThreads;
            if (i < p.n_words) __builtin_nontemporal_store(v[u], o + i);
        }
    }
}

}  // namespace rama
