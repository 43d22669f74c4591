// q8_tree_attn_body.hpp -- the body of attention_tree_kernel and attention_draft_tree_kernel (q8_tree.hpp), included once into each: the two
// differ only in RAMA_TREE_ROW, the row of tp.kr / tp.v that a path's nibble names -- the nibble itself where the rows are the pass's own, and
// nibble - 1 where they are a tree store's and the nibble is a node.  No include guard: it is included twice.
    RAMA_NO_CONTRACT
    RefAttnParams p = tp.a;
    const int y = blockIdx.y, h = blockIdx.x;
    const int pos = p.seqs[y].pos;
    if (pos < 0) return;                                          // an idle row (uniform: the whole workgroup)
    constexpr int T = NW * 64;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ SeqSumShared<NW> sh;
    __shared__ PredShared<NW> ps;
    __shared__ FastSumShared<NW> fsn;
    __shared__ float red[16];
    __shared__ unsigned long long s_tab[32];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    exp_tab_fill(s_tab);
    const int lds_seq = p.seq_len;
    const unsigned long long path = tp.anc[y].path;
    const int P = pos - tp.anc[y].depth;                          // the root's position: rows 0..P come from the cache
    const float* kcl = p.seqs[y].kc + p.layer_off;
    const float* vcl = p.seqs[y].vc + p.layer_off;
    p.q += (size_t)y * p.tok_stride; p.xb += (size_t)y * p.tok_stride;
    if (p.att) p.att += (size_t)y * p.att_stride;
    const int hs = p.head_size, hs4 = hs >> 2;
    const size_t col = (size_t)h * hs;
    // timestep t <= pos of this row, as a 16-byte pointer to its head columns: the cache's row or an ancestor's
    auto row_of = [&](const float* cache, const float* rows, int t) -> gf4p {
        const int k = max(t - P, 0);                              // 0..depth <= 15
        const int r = RAMA_TREE_ROW((int)((path >> (4 * k)) & 15ull));
        const gf4p c = gptr4(cache + (size_t)min(t, P) * p.dim + col);
        const gf4p s = gptr4(rows + (size_t)r * p.dim + col);
        return t <= P ? c : s;
    };
    float* s_q = sm;                                              // [hs]
    float* s_p = sm + ((hs + 3) & ~3);                            // [lds_seq] the probabilities
    float* s_att = s_p + ((lds_seq + 3) & ~3);                    // [scan_slot(lds_seq)] scores -> exponentials
    const int region_off = (((hs + 3) & ~3) + ((lds_seq + 3) & ~3) + lds_seq + (lds_seq >> 5) + 4 + 3) & ~3;      // (an offset, not a rounded pointer)
    float* region = sm + region_off;
    for (int i = tid; i < hs; i += T) s_q[i] = p.q[col + i];
    constexpr int U = NW >= 16 ? 4 : 8;
    const int tile4 = kAttTile * hs4;
    int er[U], ec[U];
#pragma unroll
    for (int u = 0; u < U; u++) { const int e = tid + u * T; er[u] = e / hs4; ec[u] = e - er[u] * hs4; }
    auto vissue = [&](int t0, f4 (&vr)[U]) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int tr = min(t0 + er[u], pos), c4 = ec[u];      // (rows behind pos are clamped: their products are written, never added)
            vr[u] = __builtin_nontemporal_load(row_of(vcl, tp.v, tr) + c4);
        }
    };
    f4 va[U], vb[U];
    __syncthreads();
    const float scale_div = sqrtf((float)hs);
    const f4* q4 = reinterpret_cast<const f4*>(s_q);
    if (hs % kAttPiece == 0 && pos >= 1024) {       // long contexts: staged pieces; a group of 64 timesteps may hold cache rows and ancestors
        float* stage = region + wave * (64 * kAttStride);
        const int npiece = hs / kAttPiece;
        const int lrow = lane >> 3, lc4 = lane & 7;
        const int ngroup = (pos + 64) >> 6;
        const int nstep = ((ngroup - wave + NW - 1) / NW) * npiece;
        auto load_step = [&](int st, f4 (&d)[8]) {
            const int sc = min(st, max(nstep - 1, 0));
            const int g = wave + (sc / npiece) * NW, pc = sc % npiece;
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int t = min(g * 64 + u * 8 + lrow, pos);
                d[u] = __builtin_nontemporal_load(row_of(kcl, tp.kr, t) + pc * (kAttPiece / 4) + lc4);
            }
        };
        constexpr int NB = NW >= 16 ? 1 : 2;
        f4 na[8], nb[NB == 2 ? 8 : 1];
        load_step(0, na);
        if constexpr (NB == 2) load_step(1, nb);
        float acc = 0.0f;
        auto consume = [&](int st, f4 (&d)[8]) {
#pragma unroll
            for (int u = 0; u < 8; u++) *reinterpret_cast<f4*>(stage + (u * 8 + lrow) * kAttStride + 4 * lc4) = d[u];
            load_step(st + NB, d);
            __builtin_amdgcn_wave_barrier();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const int pc = st % npiece;
            const f4* row = reinterpret_cast<const f4*>(stage + lane * kAttStride);
            f4 kk[8];
#pragma unroll
            for (int i = 0; i < 8; i++) kk[i] = row[i];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const f4 qq = q4[pc * 8 + i];
                acc = acc + qq.x * kk[i].x; acc = acc + qq.y * kk[i].y; acc = acc + qq.z * kk[i].z; acc = acc + qq.w * kk[i].w;
            }
            if (pc + 1 == npiece) {
                const int t = (wave + (st / npiece) * NW) * 64 + lane;
                if (t <= pos) s_att[scan_slot(t)] = acc / scale_div;
                acc = 0.0f;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
        };
        for (int st = 0; st < nstep; st += NB) {                  // uniform per wave
            consume(st, na);
            if constexpr (NB == 2) { if (st + 1 < nstep) consume(st + 1, nb); }
        }
    } else {
        for (int t = tid; t <= pos; t += T) {
            const gf4p k4 = row_of(kcl, tp.kr, t);
            float acc = 0.0f;
            int i = 0;
            auto batch = [&](auto nb) {
                constexpr int NB = decltype(nb)::value;
                for (; i + NB <= hs4; i += NB) {
                    f4 kk[NB];
#pragma unroll
                    for (int u = 0; u < NB; u++) kk[u] = k4[i + u];
#pragma unroll
                    for (int u = 0; u < NB; u++) {
                        const f4 qq = q4[i + u];
                        acc = acc + qq.x * kk[u].x; acc = acc + qq.y * kk[u].y; acc = acc + qq.z * kk[u].z; acc = acc + qq.w * kk[u].w;
                    }
                }
            };
            if constexpr (NW < 16) batch(std::integral_constant<int, 32>{});
            batch(std::integral_constant<int, 16>{});
            batch(std::integral_constant<int, 8>{});
            batch(std::integral_constant<int, 4>{});
            for (; i < hs4; i++) {
                const f4 kk = k4[i], qq = q4[i];
                acc = acc + qq.x * kk.x; acc = acc + qq.y * kk.y; acc = acc + qq.z * kk.z; acc = acc + qq.w * kk.w;
            }
            s_att[scan_slot(t)] = acc / scale_div;
        }
    }
    __syncthreads();
    // softmax_num (cpu.rs:187-192)
    float mx = -INFINITY;
    for (int t = tid; t <= pos; t += T) mx = fmaxf(mx, s_att[scan_slot(t)]);
    mx = block_max(mx, red);
    for (int t = tid; t <= pos; t += T) s_att[scan_slot(t)] = expf_glibc_tab(s_att[scan_slot(t)] - mx, s_tab);
    __syncthreads();
    const float sum = seq_sum_cascade<NW>(s_att, pos + 1, fsn, ps, sh);
    for (int t = tid; t <= pos; t += T) {
        const float a = s_att[scan_slot(t)] / sum;
        s_p[t] = a;
        if (p.att) p.att[(size_t)h * p.seq_len + t] = a;
    }
    float acc = 0.0f;
    vissue(0, va);
    if (pos >= kAttTile) vissue(kAttTile, vb);                   // (uniform)
    __syncthreads();                                              // the probabilities are final; the staging region is free
    auto vtile = [&](int t0, int buf, f4 (&vr)[U]) {
        float* tile = region + buf * (kAttTile * hs);
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int e = tid + u * T;
            if (e < tile4) {
                const float a = s_p[min(t0 + er[u], pos)];
                const f4 vv = vr[u];
                f4 pr;
                pr.x = a * vv.x; pr.y = a * vv.y; pr.z = a * vv.z; pr.w = a * vv.w;     // cpu.rs:48 `a * vi`, rounded
                *reinterpret_cast<f4*>(tile + 4 * e) = pr;
            }
        }
        if (t0 + 2 * kAttTile <= pos) vissue(t0 + 2 * kAttTile, vr);      // (uniform)
        __syncthreads();
        if (tid < hs) {
            const int nt = min(kAttTile, pos + 1 - t0);
            int r = 0;
            for (; r + 16 <= nt; r += 16) {
                float v16[16];
#pragma unroll
                for (int u = 0; u < 16; u++) v16[u] = tile[(r + u) * hs + tid];
#pragma unroll
                for (int u = 0; u < 16; u++) acc = acc + v16[u];
            }
            for (; r < nt; r++) acc = acc + tile[r * hs + tid];
        }
    };
    for (int t0 = 0; t0 <= pos; t0 += 2 * kAttTile) {
        vtile(t0, 0, va);
        if (t0 + kAttTile <= pos) vtile(t0 + kAttTile, 1, vb);    // uniform
    }
    if (tid < hs) p.xb[col + tid] = acc;
