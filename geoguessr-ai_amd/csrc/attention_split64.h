// fp32 attention of head dim 64 and ANY sequence length on the bf16 matrix pipe (included by attention_flash.hip after attention_split.h, inside its anonymous
// namespace): the CLIP vision tower's attention in the fp32_split mode (50 tokens: ViT-B/32; 577: ViT-L/14-336).  No bias, no windows (window_size == 0).
//
// The arithmetic is attention_split.h's -- every f32 operand as three bf16 planes, a product as six v_mfma_f32_16x16x32_bf16 with the small terms first -- in
// the work decomposition of the f32 online-softmax kernels: one 256-thread workgroup per (image, head, 64-row tile), a wave per 16-row strip, the other side
// walked in tiles of 64 tokens.  A staged tile (64 tokens x 64 columns) is split ONCE on its way into LDS, as two 32-column plane images of the layout
// attention_split.h defines (image (plane, half) at (2 plane + half) * 2048 elements; sp_frag / sp_frag_t2 read it unchanged); the next tile's global loads are in
// flight, in registers, while the current one is multiplied.  Per-wave strips are split once in registers, P / dS where they are formed.
//   forward      S^T = K Q^T (swapped: a lane owns a query, the online-softmax statistics are lane-local), O^T += V^T P^T           96 MFMAs per 64 x 16 tile pair
//   dQ pass      the forward's structure: S^T and dP^T = V dO^T from the staged K / V tile, dQ^T += K^T dS^T                        144
//   dK/dV pass   a wave owns 16 keys: S = Q K^T and dP = dO V^T from the staged Q / dO tile, dV^T += dO^T P, dK^T += Q^T dS        192
// The backward is two passes everywhere (no dS hand-off, no atomics: two runs give the same bits); both recompute P from the forward's lse, with -lse joining
// the exponent after the product (attention_split.h explains why), and form delta = sum_d dO O themselves.
constexpr int SP64_HALF = 64 * 32, SP64_PL = 2 * SP64_HALF;      // elements of one 32-column image / of one plane of a 64 x 64 tile
size_t sp64_lds(int npl, bool rowstats) { return (size_t)2 * npl * SP64_PL * sizeof(bf16) + (rowstats ? 2 * 64 * sizeof(float) : 0); }

// the 512 eight-column chunks of a 64 x 64 tile over 256 threads: chunk id -> (row, chunk of the row)
struct Sp64Regs { f32x4 v[2][2]; };
__device__ __forceinline__ int sp64_chunk_off(const FlashParams& p, int i, int t0, int ldb, int colb) {
    const int id = threadIdx.x + i * 256, tok = t0 + (id >> 3);
    return tok < p.N ? tok * ldb + colb + (id & 7) * 32 : FL_OOB;
}
__device__ __forceinline__ void sp64_issue(const FlashParams& p, __amdgpu_buffer_rsrc_t rs, int t0, int ldb, int colb, Sp64Regs& r) {
#pragma unroll
    for (int i = 0; i < 2; ++i) SpLd8<float>::load(rs, sp64_chunk_off(p, i, t0, ldb, colb), r.v[i][0], r.v[i][1]);
}
template <int NPL> __device__ __forceinline__ void sp64_commit(const Sp64Regs& r, bf16* X) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int id = threadIdx.x + i * 256, row = id >> 3, ch8 = id & 7;
        const Sp8T<NPL> s = sp_split8<NPL>(r.v[i][0], r.v[i][1]);
        const int o = (ch8 >> 2) * SP64_HALF + sp_off(row, ch8 & 3);
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) *reinterpret_cast<bf16x8*>(X + pl * SP64_PL + o) = s.p[pl];
    }
}

// ------------------------------------------------------------------------------------------- forward / dQ pass
// DQ = false: out, lse.  DQ = true: dQ of the tile's queries (reads out, dout, lse).
// CAUSAL (the CLIP text tower, gg_attention_causal_fwd / _bwd): query t sees keys 0..t.  Key tiles above the query tile are not visited (the bound is the
// workgroup's own tile: the barriers stay uniform), the diagonal tile's scores above the diagonal become -inf before the running maximum / the exponent -- their
// P is an exact 0, and so is their dS.  The dQ pass also skips, on the diagonal tile, the 16-key sub-tiles wholly above the wave's own strip (wave-uniform).
template <int NPL, bool DQ, bool CAUSAL = false>
__global__ __launch_bounds__(256) void flash64_split_q_kernel(FlashParams p) {
    typedef Sp8T<NPL> Sp8;
    extern __shared__ __attribute__((aligned(16))) float fsm[];
    bf16* Kp = reinterpret_cast<bf16*>(fsm);
    bf16* Vp = Kp + NPL * SP64_PL;
    const int tile = blockIdx.x % p.ntile, wh = blockIdx.x / p.ntile;
    const int h = wh % p.nh, w = wh / p.nh;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 15, lg = lane >> 4;
    const int64_t origin = (int64_t)w * p.N;
    const int hc = h * p.head_stride;
    const int ldb = (int)p.ld * 4, ldob = (int)p.ldo * 4, lddob = (int)p.lddo * 4;
    const __amdgpu_buffer_rsrc_t rsQKV = fl_rsrc(reinterpret_cast<const float*>(p.qkv) + origin * p.ld, p.N * ldb);
    const __amdgpu_buffer_rsrc_t rsOUT = fl_rsrc(reinterpret_cast<float*>(p.out) + origin * p.ldo, p.N * ldob);
    const __amdgpu_buffer_rsrc_t rsLSE = fl_rsrc(p.lse ? p.lse + origin * p.nh : nullptr, p.lse ? p.N * p.nh * 4 : 0);
    const __amdgpu_buffer_rsrc_t rsDO = fl_rsrc(DQ ? reinterpret_cast<const float*>(p.dout) + origin * p.lddo : nullptr, DQ ? p.N * lddob : 0);
    const __amdgpu_buffer_rsrc_t rsDQKV = fl_rsrc(DQ ? reinterpret_cast<float*>(p.dqkv) + origin * p.ld : nullptr, DQ ? p.N * ldb : 0);
    Sp64Regs kr, vr;
    sp64_issue(p, rsQKV, 0, ldb, (p.k_off + hc) * 4, kr);
    sp64_issue(p, rsQKV, 0, ldb, (p.v_off + hc) * 4, vr);
    // the wave's query strip: row lr, contraction slots d = 32 half + 8 lg .., split once (the B operand of S^T; dO likewise of dP^T)
    const int qi = tile * 64 + wave * 16 + lr;
    const bool qok = qi < p.N;
    const bool live = tile * 64 + wave * 16 < p.N;                 // (wave-uniform) a strip of padding only multiplies nothing, but keeps the barriers
    Sp8 q3[2], g3[DQ ? 2 : 1];
    float nlse = 0.f, ndel = 0.f;                                  // -lse (exp2 domain), -delta of the lane's query
    {
        float dsum = 0.f;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            f32x4 lo, hi;
            SpLd8<float>::load(rsQKV, qok ? qi * ldb + (p.q_off + hc + 32 * hf + 8 * lg) * 4 : FL_OOB, lo, hi);
            q3[hf] = sp_split8<NPL>(lo, hi);
            if constexpr (DQ) {
                f32x4 glo, ghi, olo, ohi;
                SpLd8<float>::load(rsDO, qok ? qi * lddob + (h * 64 + 32 * hf + 8 * lg) * 4 : FL_OOB, glo, ghi);
                SpLd8<float>::load(rsOUT, qok ? qi * ldob + (h * 64 + 32 * hf + 8 * lg) * 4 : FL_OOB, olo, ohi);
                g3[hf] = sp_split8<NPL>(glo, ghi);
#pragma unroll
                for (int j = 0; j < 4; ++j) dsum = fmaf(glo[j], olo[j], dsum);
#pragma unroll
                for (int j = 0; j < 4; ++j) dsum = fmaf(ghi[j], ohi[j], dsum);
            }
        }
        if constexpr (DQ) {
            dsum += __shfl_xor(dsum, 16, 64);
            dsum += __shfl_xor(dsum, 32, 64);
            ndel = -dsum;
            nlse = -1.4426950408889634f * __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsLSE, qok ? (qi * p.nh + h) * 4 : FL_OOB, 0, 0));
        }
    }
    const float sc2 = p.scale * 1.4426950408889634f;
    float mx = -INFINITY, l = 0.f;
    f32x4 acc[4];                                                  // O^T / dQ^T [d = 16 c + 4 lg + r][q = lr]
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int nt = CAUSAL ? tile + 1 : p.ntile;                    // key tiles this workgroup walks
    for (int t = 0; t < nt; ++t) {
        const int t0 = t * 64;
        __syncthreads();                                           // every wave is done with the previous tile's images
        sp64_commit<NPL>(kr, Kp);
        sp64_commit<NPL>(vr, Vp);
        __syncthreads();
        if (t + 1 < nt) {
            sp64_issue(p, rsQKV, t0 + 64, ldb, (p.k_off + hc) * 4, kr);
            sp64_issue(p, rsQKV, t0 + 64, ldb, (p.v_off + hc) * 4, vr);
        }
        if (!live) continue;
        int nkt = min(4, (p.N - t0 + 15) >> 4);                    // 16-key sub-tiles of this tile that hold a key
        if constexpr (CAUSAL && DQ) { if (t == tile) nkt = min(nkt, wave + 1); }      // (sub-tiles above the strip's diagonal: every P is 0)
        // S^T[key][q]: lane holds keys t0 + 16 kt + 4 lg + r of query lr; padded keys are masked through the initial value
        f32x4 st[4];
        float tmax = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            f32x4 s = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (kt < nkt) {
                s = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (t0 + 16 * kt + 15 >= p.N) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) s[r] = (t0 + 16 * kt + 4 * lg + r < p.N) ? 0.f : -INFINITY;
                }
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) s = sp_mma32<NPL>(sp_frag<NPL>(Kp + hf * SP64_HALF, SP64_PL, 16 * kt + lr, lg), q3[hf], s);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[r] = DQ ? fmaf(s[r], sc2, nlse) : s[r] * sc2;      // exp2 domain; the backward's exponent is complete here
                    if constexpr (CAUSAL) { if (t == tile && t0 + 16 * kt + 4 * lg + r > qi) s[r] = -INFINITY; }      // (key 0 <= every query: the maximum stays finite)
                    tmax = fmaxf(tmax, s[r]);
                }
            }
            st[kt] = s;
        }
        if constexpr (!DQ) {
            tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            const float mnew = fmaxf(mx, tmax);                    // finite: the first tile holds key 0
            const float alpha = __builtin_amdgcn_exp2f(mx - mnew); // (first tile: exp2(-inf) = 0 on zero accumulators)
            mx = mnew;
            l *= alpha;
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = acc[c] * alpha;
        }
        // two key sub-tiles (32 keys) per product: slot j of lane group lg <-> key 16 (kt + (j >> 2)) + 4 lg + (j & 3)
#pragma unroll
        for (int kt = 0; kt < 4; kt += 2) {
            if (kt >= nkt) break;
            f32x4 e0, e1;
#pragma unroll
            for (int r = 0; r < 4; ++r) { e0[r] = __builtin_amdgcn_exp2f(st[kt][r] - (DQ ? 0.f : mx)); e1[r] = __builtin_amdgcn_exp2f(st[kt + 1][r] - (DQ ? 0.f : mx)); }
            if constexpr (!DQ) {
#pragma unroll
                for (int r = 0; r < 4; ++r) l += e0[r] + e1[r];
                const Sp8 p3 = sp_split8<NPL>(e0, e1);
#pragma unroll
                for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                    for (int c = 0; c < 2; ++c)
                        acc[2 * hf + c] = sp_mma32<NPL>(sp_frag_t2<NPL>(Vp + hf * SP64_HALF, SP64_PL, 16 * kt, 16 * kt + 16, c, lr, lg), p3, acc[2 * hf + c]);
            } else {
                // dP^T[key][q] - delta[q] = V dO^T - delta; dS^T = P^T (dP^T - delta)  (the softmax scale is applied once, to dQ)
                f32x4 d0 = {ndel, ndel, ndel, ndel}, d1 = d0;
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    d0 = sp_mma32<NPL>(sp_frag<NPL>(Vp + hf * SP64_HALF, SP64_PL, 16 * kt + lr, lg), g3[hf], d0);
                    d1 = sp_mma32<NPL>(sp_frag<NPL>(Vp + hf * SP64_HALF, SP64_PL, 16 * kt + 16 + lr, lg), g3[hf], d1);
                }
                const Sp8 s3 = sp_split8<NPL>(e0 * d0, e1 * d1);
#pragma unroll
                for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                    for (int c = 0; c < 2; ++c)
                        acc[2 * hf + c] = sp_mma32<NPL>(sp_frag_t2<NPL>(Kp + hf * SP64_HALF, SP64_PL, 16 * kt, 16 * kt + 16, c, lr, lg), s3, acc[2 * hf + c]);
            }
        }
    }
    if (!live) return;
    if constexpr (!DQ) {
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        const float inv = 1.0f / l;
#pragma unroll
        for (int c = 0; c < 4; ++c) Bld<float>::store(rsOUT, qok ? qi * ldob + (h * 64 + 16 * c + 4 * lg) * 4 : FL_OOB, acc[c] * inv);
        if (p.lse) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, mx * 0.6931471805599453f + __logf(l)), rsLSE,
                                                         (qok && lg == 0) ? (qi * p.nh + h) * 4 : FL_OOB, 0, 0);
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) Bld<float>::store(rsDQKV, qok ? qi * ldb + (p.q_off + hc + 16 * c + 4 * lg) * 4 : FL_OOB, acc[c] * p.scale);
    }
}

// ------------------------------------------------------------------------------------------- dK / dV pass
// One workgroup per (image, head, 64-key tile), a wave per 16-key strip (K / V rows split once in registers); Q and dO walk through LDS in tiles of 64 queries
// with their row scalars (-lse in the exp2 domain, -delta).  Unswapped scores: a lane owns a key, P / dS of two query sub-tiles side by side are the B operand
// of the products over the 32 queries.
// CAUSAL: key k is seen by queries k.. -- query tiles below the key tile are not visited (workgroup-uniform bound), on the diagonal tile the pairs of 16-query
// sub-tiles wholly below the wave's key strip are skipped (wave-uniform, no barrier inside) and a score with key > query becomes -inf before the exponent.
template <int NPL, bool CAUSAL = false>
__global__ __launch_bounds__(256) void flash64_split_dkv_kernel(FlashParams p) {
    typedef Sp8T<NPL> Sp8;
    extern __shared__ __attribute__((aligned(16))) float fsm[];
    bf16* Qp = reinterpret_cast<bf16*>(fsm);
    bf16* Gp = Qp + NPL * SP64_PL;                                 // dO planes
    float* lse_s = reinterpret_cast<float*>(Gp + NPL * SP64_PL);
    float* del_s = lse_s + 64;
    const int tile = blockIdx.x % p.ntile, wh = blockIdx.x / p.ntile;
    const int h = wh % p.nh, w = wh / p.nh;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 15, lg = lane >> 4;
    const int64_t origin = (int64_t)w * p.N;
    const int hc = h * p.head_stride;
    const int ldb = (int)p.ld * 4, ldob = (int)p.ldo * 4, lddob = (int)p.lddo * 4;
    const __amdgpu_buffer_rsrc_t rsQKV = fl_rsrc(reinterpret_cast<const float*>(p.qkv) + origin * p.ld, p.N * ldb);
    const __amdgpu_buffer_rsrc_t rsO = fl_rsrc(reinterpret_cast<const float*>(p.out) + origin * p.ldo, p.N * ldob);
    const __amdgpu_buffer_rsrc_t rsLSE = fl_rsrc(p.lse + origin * p.nh, p.N * p.nh * 4);
    const __amdgpu_buffer_rsrc_t rsDO = fl_rsrc(reinterpret_cast<const float*>(p.dout) + origin * p.lddo, p.N * lddob);
    const __amdgpu_buffer_rsrc_t rsDQKV = fl_rsrc(reinterpret_cast<float*>(p.dqkv) + origin * p.ld, p.N * ldb);
    Sp64Regs qr, gr, orr;
    float lsev[2];
    auto issue = [&](int t0) {
        sp64_issue(p, rsQKV, t0, ldb, (p.q_off + hc) * 4, qr);
        sp64_issue(p, rsDO, t0, lddob, h * 64 * 4, gr);
        sp64_issue(p, rsO, t0, ldob, h * 64 * 4, orr);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = threadIdx.x + i * 256, tok = t0 + (id >> 3);
            lsev[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsLSE, (tok < p.N && (id & 7) == 0) ? (tok * p.nh + h) * 4 : FL_OOB, 0, 0));
        }
    };
    const int tfirst = CAUSAL ? tile : 0;                          // query tiles this workgroup walks: tfirst .. ntile - 1
    issue(tfirst * 64);
    const int ki = tile * 64 + wave * 16 + lr;
    const bool kok = ki < p.N;
    const bool live = tile * 64 + wave * 16 < p.N;
    Sp8 k3[2], v3[2];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        f32x4 lo, hi;
        SpLd8<float>::load(rsQKV, kok ? ki * ldb + (p.k_off + hc + 32 * hf + 8 * lg) * 4 : FL_OOB, lo, hi);
        k3[hf] = sp_split8<NPL>(lo, hi);
        SpLd8<float>::load(rsQKV, kok ? ki * ldb + (p.v_off + hc + 32 * hf + 8 * lg) * 4 : FL_OOB, lo, hi);
        v3[hf] = sp_split8<NPL>(lo, hi);
    }
    const float sc2 = p.scale * 1.4426950408889634f;
    f32x4 dk[4], dv[4];                                            // dK^T / dV^T [d = 16 c + 4 lg + r][key = lr]
#pragma unroll
    for (int c = 0; c < 4; ++c) dk[c] = dv[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int t = tfirst; t < p.ntile; ++t) {
        const int t0 = t * 64;
        __syncthreads();
        sp64_commit<NPL>(qr, Qp);
        sp64_commit<NPL>(gr, Gp);
        // -delta = -sum_d dO O (the 8 threads of a row) and -lse in the exp2 domain (-inf for padded queries: their P is 0)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = threadIdx.x + i * 256, row = id >> 3;
            float dsum = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) dsum = fmaf(gr.v[i][0][j], orr.v[i][0][j], dsum);
#pragma unroll
            for (int j = 0; j < 4; ++j) dsum = fmaf(gr.v[i][1][j], orr.v[i][1][j], dsum);
            dsum += __shfl_xor(dsum, 1, 64);
            dsum += __shfl_xor(dsum, 2, 64);
            dsum += __shfl_xor(dsum, 4, 64);
            if ((id & 7) == 0) {
                del_s[row] = -dsum;
                lse_s[row] = t0 + row < p.N ? -1.4426950408889634f * lsev[i] : -INFINITY;
            }
        }
        __syncthreads();
        if (t + 1 < p.ntile) issue(t0 + 64);
        if (!live) continue;
        const int nqt = min(4, (p.N - t0 + 15) >> 4);
#pragma unroll
        for (int qt = 0; qt < 4; qt += 2) {
            if (qt >= nqt) break;
            if constexpr (CAUSAL) { if (t == tile && qt + 2 <= wave) continue; }      // every query of the pair precedes the strip's first key
            f32x4 pr[2], ds[2];                                    // lane holds [q = t0 + 16 (qt + a) + 4 lg + r][key = lr]
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int q0 = 16 * (qt + a);
                const f32x4 nl4 = *reinterpret_cast<const f32x4*>(lse_s + q0 + 4 * lg), dp0 = *reinterpret_cast<const f32x4*>(del_s + q0 + 4 * lg);
                f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = dp0;
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    s = sp_mma32<NPL>(sp_frag<NPL>(Qp + hf * SP64_HALF, SP64_PL, q0 + lr, lg), k3[hf], s);
                    dp = sp_mma32<NPL>(sp_frag<NPL>(Gp + hf * SP64_HALF, SP64_PL, q0 + lr, lg), v3[hf], dp);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float x = fmaf(s[r], sc2, nl4[r]);
                    if constexpr (CAUSAL) { if (t == tile && ki > t0 + q0 + 4 * lg + r) x = -INFINITY; }
                    const float e = __builtin_amdgcn_exp2f(x);
                    pr[a][r] = e;
                    ds[a][r] = e * dp[r];                          // (a padded key's column is finite; its dK / dV rows are dropped by the range check)
                }
            }
            const Sp8 p3 = sp_split8<NPL>(pr[0], pr[1]), s3 = sp_split8<NPL>(ds[0], ds[1]);
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    dv[2 * hf + c] = sp_mma32<NPL>(sp_frag_t2<NPL>(Gp + hf * SP64_HALF, SP64_PL, 16 * qt, 16 * qt + 16, c, lr, lg), p3, dv[2 * hf + c]);
                    dk[2 * hf + c] = sp_mma32<NPL>(sp_frag_t2<NPL>(Qp + hf * SP64_HALF, SP64_PL, 16 * qt, 16 * qt + 16, c, lr, lg), s3, dk[2 * hf + c]);
                }
        }
    }
    if (!live) return;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        Bld<float>::store(rsDQKV, kok ? ki * ldb + (p.k_off + hc + 16 * c + 4 * lg) * 4 : FL_OOB, dk[c] * p.scale);
        Bld<float>::store(rsDQKV, kok ? ki * ldb + (p.v_off + hc + 16 * c + 4 * lg) * 4 : FL_OOB, dv[c]);
    }
}
