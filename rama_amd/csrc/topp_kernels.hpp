// topp_kernels.hpp -- the samplers' kernels that are no templates (five of topp_sort.hpp, argmax_kernel, topp_pick_kernel): chain_api.hip alone launches them.
// A kernel that is no template is emitted by every translation unit that sees its definition, so these live
// apart from the types, device functions and template kernels of topp_sort.hpp, which the Q8 translation units see too (q8_serve_api.hip and q8_spec_api.hip for their pick kernels).
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

// the single-sequence samplers (from ops_kernels.hpp: every launch of them is chain_api.hip's)
__global__ __launch_bounds__(1024) void argmax_kernel(ArgmaxParams p) {
    __shared__ float s_v[16];
    __shared__ int s_i[16];
    __shared__ int s_next;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // cursor reads go out first; their latency overlaps the logits sweep
    int pos = 0, n_forced = 0, n_out = 0, forced_tok = -1;
    if (p.ctl && tid == 0) {
        pos = p.ctl->pos; n_forced = p.ctl->n_forced; n_out = p.ctl->n_out;
        if (pos < n_forced) forced_tok = p.forced[pos];
    }
    float bv = -INFINITY; int bi = -1;
    // 16-byte loads when the view is aligned; every thread visits its indices in ascending
    // order, so "replace unless strictly smaller" keeps the LAST maximum (cpu.rs:165-167)
    const int n4 = (((uintptr_t)p.logits & 15) == 0) ? (p.n >> 2) : 0;
    const f4* l4 = reinterpret_cast<const f4*>(p.logits);
    // 8 loads in flight per thread: one workgroup sweeps 128 KB, and a dependent load per iteration
    // would cost a cache round trip each (this launch is pure latency)
    for (int i0 = tid; i0 < n4; i0 += 8 * 1024) {
        f4 v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = l4[min(i0 + u * 1024, n4 - 1)];      // ([r4] clamped, not conditional: `i < n4 ? load : x` is a branch with
                                                                                  // s_waitcnt vmcnt(0) behind it -- the eight loads went out one by one)
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int i = i0 + u * 1024;
            if (i < n4) {
                if (!(bv > v[u].x)) { bv = v[u].x; bi = 4 * i; }
                if (!(bv > v[u].y)) { bv = v[u].y; bi = 4 * i + 1; }
                if (!(bv > v[u].z)) { bv = v[u].z; bi = 4 * i + 2; }
                if (!(bv > v[u].w)) { bv = v[u].w; bi = 4 * i + 3; }
            }
        }
    }
    for (int i = 4 * n4 + tid; i < p.n; i += 1024) {
        const float v = p.logits[i];
        if (!(bv > v)) { bv = v; bi = i; }
    }
    const float wm = wave_max(bv);
    const int wi = wave_max_i(bv == wm ? bi : -1);
    if (lane == 0) { s_v[wave] = wm; s_i[wave] = wi; }
    __syncthreads();
    if (tid == 0) {
        float v = s_v[0]; int idx = s_i[0];
        for (int w = 1; w < 16; w++) {
            const float ov = s_v[w]; const int oi = s_i[w];
            if (oi >= 0 && (idx < 0 || ov > v || (ov == v && oi > idx))) { v = ov; idx = oi; }
        }
        s_next = finish_step(p, idx, pos, n_forced, n_out, forced_tok);
    }
    gather_next_embedding(p, &s_next);
}

__global__ __launch_bounds__(1024) void topp_pick_kernel(ToppParams p, ArgmaxParams fin) {
    __shared__ float s_p[2][kToppChunk];
    __shared__ int s_last, s_next, s_pick;
    __shared__ float s_cum;
    const int tid = threadIdx.x;
    int pos = 0, n_forced = 0, n_out = 0, forced_tok = -1;
    if (fin.ctl && tid == 0) {
        pos = fin.ctl->pos; n_forced = fin.ctl->n_forced; n_out = fin.ctl->n_out;
        if (pos < n_forced) forced_tok = fin.forced[pos];
    }
    const int m = *p.m;
    if (tid == 0) { s_last = m > 0 ? m - 1 : 0; s_cum = 0.0f; s_pick = 0; }
    // Sequential running sum in sorted order (infer.rs:70-73): the fp32 rounding of cum_i depends
    // on every earlier add, so the chain cannot be split.  Wave 0 walks it 64 values at a time with
    // a lane ripple: lane i holds p_i, lane 0 is seeded with carry + p_0, and 63 identical
    // `v_add_f32_dpp s, s, p wave_shr:1` steps (lane i: s = s[i-1] + p_i; lane 0 has no source lane
    // and keeps its value) leave S_i in lane i -- one 4-cycle VALU op (+2 wait states) per element,
    // no LDS turn inside the chain.  All threads stage the next 4096-value chunk meanwhile (double
    // buffer) and afterwards copy the running sums out.  Padding zeros leave the sum unchanged.
    const int nchunks = (m + kToppChunk - 1) / kToppChunk;
    auto stage = [&](int c) {
        const int base = c * kToppChunk, len = min(kToppChunk, m - base), padded = (len + 63) & ~63;
        for (int i = tid; i < padded; i += 1024) s_p[c & 1][i] = i < len ? p.keys[base + i] : 0.0f;
    };
    if (nchunks > 0) stage(0);
    __syncthreads();
    for (int c = 0; c < nchunks; c++) {
        const int base = c * kToppChunk, len = min(kToppChunk, m - base);
        if (c + 1 < nchunks) stage(c + 1);
        if (tid < 64) {
            float* q = s_p[c & 1];
            float carry = s_cum;
            const int nblk = (len + 63) >> 6;
            int hit = -1;
            float pv = q[tid];
            for (int blk = 0; blk < nblk; blk++) {
                const float pn = q[min(blk + 1, nblk - 1) * 64 + tid];      // next block's values: in flight during the ripple
                float sv = tid == 0 ? carry + pv : pv;
#pragma unroll
                for (int k = 0; k < 63; k++)
                    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %1 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(sv) : "v"(pv));
                q[blk * 64 + tid] = sv;
                carry = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, sv), 63));
                const unsigned long long over = __ballot(sv > p.topp);
                if (over) {                       // sums are non-decreasing: the first set lane is the crossing
                    const int l0 = __ffsll((long long)over) - 1;
                    hit = blk * 64 + l0;
                    carry = __shfl(sv, l0);
                    break;
                }
                pv = pn;
            }
            if (tid == 0) {
                s_cum = carry;
                if (hit >= 0) { s_last = base + hit; s_pick = 1; }
            }
        }
        __syncthreads();
        // running sums of this chunk -> global (read again below); only indices < last matter
        for (int i = tid; i < len; i += 1024) p.prefix[base + i] = s_p[c & 1][i];
        if (s_pick) break;                                   // uniform
        __syncthreads();
    }
    __syncthreads();
    // r = u * cum; the first i < last whose running sum exceeds r wins, else `last` (infer.rs:75-84);
    // the running sums of that loop are exactly the ones stored above
    const int last = s_last;
    const float r = p.u * s_cum;
    // the running sums never decrease, so "first i < last with r < cum_i" = the number of i < last
    // with cum_i <= r: independent loads, no early exit
    int below = 0;
    for (int i = tid; i < last; i += 1024) below += !(r < p.prefix[i]);
    const int best = min(block_sum_i(below), last);
    if (tid == 0) {
        const int idx = m > 0 ? p.vals[best] : -1;
        s_next = finish_step(fin, idx, pos, n_forced, n_out, forced_tok);
    }
    gather_next_embedding(fin, &s_next);
}

}  // namespace rama
