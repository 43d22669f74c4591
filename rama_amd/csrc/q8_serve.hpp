// q8_serve.hpp -- the SERVING CHAIN of a Q8 model (rama_q8_serve_begin / _admit / _steps): continuous
// batching on the device.  n_slots sequence slots share weight passes of max_rows rows.  Every step
//   serve_schedule_kernel   slot table -> row table (SeqSlot[max_rows]: cache bases, position, slot), row tokens, per slot its row
//                           count, its logits row and the sampler record of the step; the row counters
//   the batched pass        q8_batch_layers over max_rows rows (an idle row has position -1: its RoPE / cache-write and attention
//                           workgroups return before they touch a pointer; products, norms and the quantizer are row-local)
//   serve_gather_kernel     the <= n_slots rows that carry logits -> a compact buffer; final norm, quantizer, classifier on those
//   the batched sampler's ordering launches (topp_sort.hpp; a slot without logits or at temperature 0 leaves them at once)
//   serve_pick_kernel       one workgroup per slot: argmax / top-p pick, then the slot's state machine
// and between any two steps serve_install_kernel puts a new sequence into a slot and serve_cancel_kernel ends the occupants of a set of
// slots (both stream-ordered, the captured step untouched).
//
// The scheduling rule (rama_q8_serve_plan_step is the same rule on the host; the two tables must be identical):
//   every DECODE slot one row (its token at its position); every PROMPT slot one row (its next context position); the rows left
//   over go to the PROMPT slots in ascending slot index, each taking as many further consecutive context positions as it has and
//   as fit; the rest are idle.  Rows are laid out by slot index, a slot's rows at consecutive positions, idle rows last.
// Several rows of one slot in one step: the RoPE launch writes their cache rows before the attention launch reads them, and a
// (head, row) workgroup at position p reads rows 0..p of its own slot only -- what rama_q8_prefill's passes rely on.
#pragma once
#define RAMA_Q8_SERVE_HPP 1     // (q8_api.hip and q8_spec_api.hip refuse to be compiled with this header: its kernels are q8_serve_api.hip's)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "topp_sort.hpp"
#include "q8_serve_tables.hpp"

namespace rama {

// exclusive sum over the 128 threads of the workgroup (and the total)
__device__ __forceinline__ unsigned long long serve_scan128(unsigned long long v, unsigned long long* buf, unsigned long long* total) {
    const int tid = threadIdx.x;
    buf[tid] = v;
    __syncthreads();
    for (int d = 1; d < kServeMaxSlots; d <<= 1) {
        const unsigned long long x = tid >= d ? buf[tid - d] : 0ull;
        __syncthreads();
        buf[tid] += x;
        __syncthreads();
    }
    const unsigned long long inc = buf[tid];
    *total = buf[kServeMaxSlots - 1];
    __syncthreads();
    return inc - v;
}

__global__ __launch_bounds__(kServeMaxSlots) void serve_schedule_kernel(ServeTables t) {
    __shared__ unsigned long long s_buf[kServeMaxSlots];
    __shared__ int s_off[kServeMaxSlots + 1];
    const int i = threadIdx.x;
    ServeSlot s{};
    if (i < t.n_slots) s = t.slots[i];
    const bool dec = s.state == kServeDecode, pro = s.state == kServePrompt;
    const int base = dec || pro ? 1 : 0;
    const int want = pro ? s.n_ctx - s.cursor - 1 : 0;            // context positions beyond the slot's first row
    // one scan for three sums: slots with a row (bits 52..), DECODE slots (bits 40..51), further positions wanted (bits 0..39)
    unsigned long long tot;
    const unsigned long long before = serve_scan128(((unsigned long long)base << 52) | ((unsigned long long)(dec ? 1 : 0) << 40) | (unsigned long long)want, s_buf, &tot);
    const int n_base = (int)(tot >> 52), n_dec = (int)((tot >> 40) & 0xFFFull);
    const long long want_before = (long long)(before & ((1ull << 40) - 1ull));
    const long long left = (long long)(t.max_rows - n_base) - want_before;       // rows left over when this slot's turn comes
    const int extra = left <= 0 ? 0 : (int)((long long)want < left ? (long long)want : left);
    const int n = base + extra;
    const int off = (int)serve_scan128((unsigned long long)n, s_buf, &tot);
    const int used = (int)tot;
    if (i < t.n_slots) {
        const bool lg = dec || (pro && s.cursor + n == s.n_ctx);  // a DECODE row, or the final context position
        t.nrows[i] = n;
        t.lrow[i] = lg ? off + n - 1 : -1;
        t.trow[i] = ToppRow{lg ? s.temperature : 0.0f, s.topp, s.u, 0, nullptr};
    }
    s_off[i] = off;
    if (i == kServeMaxSlots - 1) s_off[kServeMaxSlots] = used;
    __syncthreads();
    if (i < t.max_rows) {
        if (i < used) {
            int lo = 0, hi = kServeMaxSlots - 1;                  // the first slot whose rows end behind row i
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_off[mid + 1] > i) hi = mid; else lo = mid + 1; }
            const ServeSlot o = t.slots[lo];
            const int pos = o.cursor + (i - s_off[lo]);
            t.rows[i] = SeqSlot{o.kc, o.vc, pos, lo};
            t.row_tok[i] = o.state == kServeDecode ? o.tok : t.ctx[(size_t)lo * t.seq_len + pos];
        } else {
            t.rows[i] = SeqSlot{nullptr, nullptr, -1, -1};
            t.row_tok[i] = 0;
        }
    }
    if (i == 0) {
        t.counters[0] += 1ull;
        t.counters[1] += (unsigned long long)n_dec;
        t.counters[2] += (unsigned long long)(used - n_dec);
        t.counters[3] += (unsigned long long)(t.max_rows - used);
    }
}

// X[r] = token_embedding_table[row_tok[r]] for the rows of the step's table that some slot wants (the fp32 chain's pass, batch_api.hip: an idle
// row keeps what it holds, so a tile nobody wants is not touched at all)
__global__ void serve_embed_rows_kernel(float* X, const float* emb, const int* row_tok, const SeqSlot* rows, int dim) {
    const int r = blockIdx.y;
    if (rows[r].pos < 0) return;                                  // (uniform: the whole workgroup)
    const size_t base = (size_t)row_tok[r] * dim;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < dim; k += gridDim.x * blockDim.x) X[(size_t)r * dim + k] = emb[base + k];
}

// XG[s] = X[the slot's logits row] (row 0 for a slot without one: a harmless row the pick skips)
__global__ void serve_gather_kernel(float* XG, const float* X, const int* lrow, int dim) {
    const int s = blockIdx.y;
    const int r = max(lrow[s], 0);
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < dim; k += gridDim.x * blockDim.x) XG[(size_t)s * dim + k] = X[(size_t)r * dim + k];
}

// an admission: the record (a ServeSlot, then n_ctx context tokens) that an async copy has brought to `rec`
__global__ void serve_install_kernel(ServeTables t, int slot, const ServeSlot* rec) {
    const int* toks = reinterpret_cast<const int*>(rec + 1);
    const int n = rec->n_ctx;
    for (int k = threadIdx.x; k < n; k += blockDim.x) t.ctx[(size_t)slot * t.seq_len + k] = toks[k];
    if (threadIdx.x == 0) t.slots[slot] = *rec;
}

// a cancel (rama_q8_serve_cancel / rama_serve_cancel): one workgroup of kServeMaxSlots threads, thread i is slot i; the set is a
// 128-bit mask in two launch arguments (nothing to stage).  A PROMPT or DECODE slot of the set becomes DONE -- to every kernel of a step what a
// slot is that ran out of budget here -- and its finished word RAMA_SERVE_CANCELLED; cursor, n_out, tok, out, the ring and the caches stay.
// A slot in any other state is left alone: an occupant that finished by itself keeps its word 1.
constexpr int kServeCancelled = 2;
__global__ __launch_bounds__(kServeMaxSlots) void serve_cancel_kernel(ServeTables t, unsigned long long lo, unsigned long long hi) {
    const int i = threadIdx.x;
    if (i >= t.n_slots) return;
    if (!(((i < 64 ? lo : hi) >> (i & 63)) & 1ull)) return;
    ServeSlot* d = t.slots + i;
    const int state = d->state;
    if (state != kServePrompt && state != kServeDecode) return;
    d->state = kServeDone;
    // (the ring words of the steps before are this stream's earlier kernels' stores: who sees the word set finds every token)
    __hip_atomic_store(t.done + i, kServeCancelled, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// What ends a step, one workgroup per slot.  A PROMPT slot still inside its context moves its cursor on; a slot with logits takes
// Device::sample -- the argmax (cpu.rs:163-167: the LAST maximal index) or topp_pick_scan_kernel's pick on the slices the
// ordering launches left -- records the token as batch_seq_advance does (out, the host-visible ring word, then the finished word),
// and becomes DECODE, or DONE on its max_new-th token or a sampled stop token.
struct ServePickParams {
    ServeTables t;
    PickRows r;                                    // one row per slot
};
__global__ __launch_bounds__(1024) void serve_pick_kernel(ServePickParams p) {
    __shared__ ScanShared sh;
    __shared__ float s_v[16];
    __shared__ int s_i[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const ServeSlot s = p.t.slots[b];
    const int n = p.t.nrows[b], lr = p.t.lrow[b];
    if (n == 0) return;                                            // FREE or DONE (uniform: the whole workgroup)
    if (lr < 0) {                                                  // inside its context: no logits yet
        __syncthreads();                                           // every thread has read the slot before it changes
        if (tid == 0) p.t.slots[b].cursor = s.cursor + n;
        return;
    }
    const int next = topp_row_pick(p.r, b, s.temperature, s.topp, s.u, sh, s_v, s_i);
    __syncthreads();
    if (tid != 0) return;
    const int k = s.n_out;
    ServeSlot* d = p.t.slots + b;
    p.t.out[(size_t)b * p.t.out_cap + k] = next;
    // the host may be polling this word while the chain runs on: one system-scope store
    __hip_atomic_store(p.t.ring + (size_t)b * p.t.out_cap + k, next + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    d->n_out = k + 1;
    d->tok = next;
    d->cursor = s.cursor + n;                                      // PROMPT: n_ctx, the first generated position; DECODE: one on
    if (k + 1 >= s.max_new || next == s.stop) {
        d->state = kServeDone;
        __hip_atomic_store(p.t.done + b, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);      // (after the ring word: who sees it set finds every token)
    } else {
        d->state = kServeDecode;
    }
}

}  // namespace rama
