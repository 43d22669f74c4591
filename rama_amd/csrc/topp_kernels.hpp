// topp_kernels.hpp -- the kernels of topp_sort.hpp that are no templates: rama_api.hip alone launches them.
// A kernel that is no template is emitted by every translation unit that sees its definition, so these live
// apart from the types, device functions and template kernels of topp_sort.hpp, which q8_api.hip sees too.
#pragma once
#include "topp_sort.hpp"

namespace rama {

// The ranking spread over the chip (round 4).  topp_rank_kernel holds ALL sorted blocks in one workgroup's LDS and lets each of its
// 1 024 threads search the 15 other blocks: 169 000 conflicting LDS probes on ONE CU per workgroup, 32 CUs busy, the last wave out at
// 21.8 us (tools/topp_bench.hip).  Here a workgroup is a PAIR (b, o): it stages block o alone (8 KB), every entry of block b does ONE
// binary search in it, and the count goes into the entry's accumulator with an integer atomic -- nblk x (nblk - 1) workgroups of
// 22 000 probes each, all CUs busy; topp_rank_scatter_kernel then puts (p, index) at place = own place in the block + the sum.
__global__ __launch_bounds__(1024) void topp_rank_pairs_kernel(ToppSortParams p) {
    __shared__ unsigned s_o[kToppBlock];
    const int tid = threadIdx.x;
    const int b = blockIdx.x, o = blockIdx.y;
    if (b == o) return;
    const int cb = p.bcount[b], co = p.bcount[o];
    if (cb == 0 || co == 0) return;                                // uniform
    const unsigned k0 = tid < cb ? __float_as_uint(p.bp[(size_t)b * kToppBlock + tid]) : 0u;
    const unsigned k1 = tid + 1024 < cb ? __float_as_uint(p.bp[(size_t)b * kToppBlock + 1024 + tid]) : 0u;
    {
        const unsigned v0 = tid < co ? __float_as_uint(p.bp[(size_t)o * kToppBlock + tid]) : 0u;
        const unsigned v1 = tid + 1024 < co ? __float_as_uint(p.bp[(size_t)o * kToppBlock + 1024 + tid]) : 0u;
        s_o[tid] = v0; s_o[tid + 1024] = v1;
    }
    __syncthreads();
    // entries of block o that precede mine: "precedes" holds on a prefix of the sorted block, so the count grows by every power of
    // two whose last covered entry still precedes (equal probabilities: the earlier block's entry comes first)
    int top = 1;
    while (top <= co) top <<= 1;                                   // uniform
    int p0 = 0, p1 = 0;
    for (int step = top >> 1; step >= 1; step >>= 1) {
        const unsigned q0 = s_o[min(p0 + step - 1, kToppBlock - 1)], q1 = s_o[min(p1 + step - 1, kToppBlock - 1)];
        const bool pr0 = o < b ? q0 >= k0 : q0 > k0, pr1 = o < b ? q1 >= k1 : q1 > k1;
        p0 += (p0 + step <= co && pr0) ? step : 0;
        p1 += (p1 + step <= co && pr1) ? step : 0;
    }
    if (tid < cb && p0) atomicAdd(&p.racc[(size_t)b * kToppBlock + tid], p0);
    if (tid + 1024 < cb && p1) atomicAdd(&p.racc[(size_t)b * kToppBlock + 1024 + tid], p1);
}

__global__ __launch_bounds__(1024) void topp_rank_scatter_kernel(ToppSortParams p) {
    const int g = blockIdx.x * 1024 + threadIdx.x;
    const int b = g / kToppBlock, s = g % kToppBlock;
    if (g == 0) {
        int total = 0;
        for (int o = 0; o < p.nblk; o++) total += p.bcount[o];
        *p.m = total;
        if (total == 0 && p.err) *p.err = 1u;
    }
    if (b >= p.nblk || s >= p.bcount[b]) return;
    const int rank = s + p.racc[(size_t)b * kToppBlock + s];
    p.keys[rank] = p.bp[(size_t)b * kToppBlock + s];
    p.vals[rank] = p.bi[(size_t)b * kToppBlock + s];
}

// The same ranking for ANY number of blocks (vocabularies above 32768 entries; rama_set_tuning "topp_sort" = 0 anywhere):
// the other blocks' sorted probabilities are probed in global memory (L2) instead of LDS, eight blocks' probes of a
// step in flight together.  Replaces the library radix sort of rounds 1-2: no library kernel is left in the product.
__global__ __launch_bounds__(256) void topp_rank_global_kernel(ToppSortParams p) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int b = g / kToppBlock, s = g % kToppBlock;              // b is uniform over the workgroup (2048 % 256 == 0)
    if (g == 0) {
        int total = 0;
        for (int o = 0; o < p.nblk; o++) total += p.bcount[o];
        *p.m = total;
        if (total == 0 && p.err) *p.err = 1u;
    }
    if (b >= p.nblk) return;
    const int mine = p.bcount[b];
    if (s >= mine) return;
    const unsigned key = __float_as_uint(p.bp[(size_t)b * kToppBlock + s]);
    int rank = s;
    for (int o0 = 0; o0 < p.nblk; o0 += 8) {
        int cnt[8], pos[8];
#pragma unroll
        for (int q = 0; q < 8; q++) { const int o = o0 + q; cnt[q] = (o < p.nblk && o != b) ? p.bcount[o] : 0; pos[q] = 0; }
        for (int step = kToppBlock; step >= 1; step >>= 1) {         // pos grows by every power of two whose last covered entry still precedes
            unsigned probe[8];
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int o = o0 + q;
                const int j = min(pos[q] + step - 1, kToppBlock - 1);
                probe[q] = cnt[q] > 0 ? __float_as_uint(p.bp[(size_t)min(o, p.nblk - 1) * kToppBlock + j]) : 0u;
            }
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int o = o0 + q;
                const bool precedes = o < b ? probe[q] >= key : probe[q] > key;
                pos[q] += (pos[q] + step <= cnt[q] && precedes) ? step : 0;
            }
        }
#pragma unroll
        for (int q = 0; q < 8; q++) rank += pos[q];
    }
    p.keys[rank] = __uint_as_float(key);
    p.vals[rank] = p.bi[(size_t)b * kToppBlock + s];
}

__global__ __launch_bounds__(1024) void topp_pick_scan_kernel(ToppParams p, ArgmaxParams fin) {
    __shared__ ScanShared sh;
    topp_pick_scan_body(p, fin, sh);
}

__global__ __launch_bounds__(1024) void topp_pick_batch_kernel(ToppBatchParams p) {
    __shared__ ScanShared sh;
    __shared__ float s_v[16];
    __shared__ int s_i[16];
    const int row = blockIdx.x, tid = threadIdx.x;
    if (p.seqs && batch_seq_finished(row, p.seqs, p.ends)) return;      // (uniform: the whole workgroup)
    const ToppRow r = p.rows[row];
    const int pos = p.seqs ? p.seqs[row].pos : 0;
    const bool forced = p.seqs && pos < r.n_forced;
    int idx;
    if (forced) idx = r.forced[pos];                              // uniform branches: the row's mode
    else if (r.temperature == 0.0f) idx = topp_row_argmax(p.logits + (size_t)row * p.ld, p.n, s_v, s_i);
    else {
        const size_t o = (size_t)row * p.rstride;
        ToppParams tp{};
        tp.logits = p.logits + (size_t)row * p.ld; tp.n = p.n; tp.temperature = r.temperature; tp.topp = r.topp; tp.u = r.u;
        tp.keys = p.keys + o; tp.vals = p.vals + o; tp.m = p.m + row;
        ArgmaxParams fin{};
        fin.result = &s_i[0];                                      // finish_step's raw pick (-1: nothing kept)
        topp_pick_scan_body(tp, fin, sh);
        __syncthreads();
        idx = s_i[0];
    }
    __syncthreads();                                               // every wave has read the position before it moves on
    if (tid != 0) return;
    if (!p.seqs) { p.result[row] = idx; return; }
    batch_seq_advance(row, idx < 0 ? 0 : idx, pos, forced, p.toks, p.seqs, p.out, p.out_cap, p.ring, p.ends);
}

}  // namespace rama
