// CLIP vision tower (transformers CLIPVisionModel as the reference uses it): forward for the embedder
// (pretrain/clip_embedder.py:51-66: base_model(pixel_values).last_hidden_state.mean(dim=1), no post_layernorm) and forward + backward
// for SuperGuessr with a CLIP base (models/super_guessr.py:134-150,323-325: the last encoder layer is fine-tuned when the pretrained
// head exists, every layer otherwise; main_coordinator_idun_s3.py:183-203 builds that model for training).
//
// A static schedule of libgg launches on one stream, in one of five arithmetic modes (GgClipCfg.act_dtype):
//   1  fp32 -- the reference's precision: f32 activations, v_mfma_f32_16x16x4_f32 GEMMs (gg_gemm_nt_f32 / gg_gemm_tn_f32), f32 LayerNorm, f32
//      online-softmax attention (head dim 64);
//   3  fp32_split -- mode 1's storage and workspace; every GEMM as an f32-accurate split product on the bf16 MFMA (x = x1 + x2 + x3 in bf16, six
//      v_mfma_f32_16x16x32_bf16 per f32 product): forward and data gradients through gg_gemm_nt_split3_af32 against cached weight planes, weight
//      gradients through gg_gemm_tn_split3, attention through the split kernels of attention_split64.h (gg_attention_flash_fwd / _bwd, dtype 3);
//      LayerNorm, token assembly, column sums and pooling are mode 1's f32 kernels;
//   0  bf16 -- bf16 activations / MFMA operands, f32 accumulation, f32 statistics;
//   2  fp16 -- the same with fp16 storage / v_mfma_f32_16x16x32_f16 (BASELINE config c4 names fp16), inference only;
//   8  fp8 -- mode 2's storage and schedule with the four Linears of every encoder layer (qkv, out_proj, fc1, fc2) as W8A8 e4m3 products
//      (include/gg_fp8.h: one f32 scale per token row and per output channel, v_mfma_scale_f32_16x16x128_f8f6f4); LN1 / LN2 leave codes + scales directly,
//      the attention output and the QuickGELU output are quantised by a pass of their own.  The vision tower only, inference only.
// Patch embedding is a pure GEMM (stride == kernel); q/k/v projections are one [3D, D] GEMM; QuickGELU rides on fc1's epilogue (with the
// pre-activation copy the backward pass needs), residual adds on out_proj's and fc2's.  Training keeps, for every layer from the first
// trainable one up, the tensors its backward pass reads (layer input, both LayerNorm outputs + statistics, qkv, attention output + row
// log-sum-exp, fc1 pre-activation and activation): sized for HBM, nothing is recomputed.  Frozen layers below run in place on scratch.
// With activation recompute (GgClipCfg.recompute = 1) those layers keep only their input: everything else of a layer lives in ONE layer-sized
// segment region all of them share, and the backward runs a layer's forward body again (the same launches on the same inputs) right before that
// layer's backward -- the top layer excepted, whose tensors are still in the region from the forward.
#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include <string.h>
#include <stdio.h>
#include "common.h"
#include "../../include/gg.h"
#include "../../include/gg_clip_text.h"
#include "../../include/gg_clip_text_train.h"
#include "../../include/gg_fp8.h"
#include "../../include/gg_attn16.h"
#include "../../include/gg_attn16b.h"
#include "../../include/gg_clip_interp.h"
#include "attention_route.h"
#include <atomic>

namespace {
struct TInfo { std::string name; int64_t offset, numel; int ndim; int64_t shape[4]; };
struct LayerP {
    int q_w, q_b, k_w, k_b, v_w, v_b, o_w, o_b, ln1_g, ln1_b, fc1_w, fc1_b, fc2_w, fc2_b, ln2_g, ln2_b;      // tensor ids
    int64_t wqkv, bqkv, wqkvT, wo, woT, w1, w1T, w2, w2T;                                                     // weight-cache offsets
    int64_t wqkv3 = -1, wqkvT3 = -1, wo3 = -1, woT3 = -1, w13 = -1, w1T3 = -1, w23 = -1, w2T3 = -1;           // fp32_split: bf16 planes [3][N][K] of the same matrices
    int64_t wqkv8 = -1, wo8 = -1, w18 = -1, w28 = -1, sqkv = -1, so = -1, s1 = -1, s2 = -1;                   // fp8: e4m3 images [N][K] of the forward matrices and their f32 scales [N]
};
struct CModel {
    GgClipCfg cfg;
    std::vector<TInfo> t;
    int64_t floats = 0, wc_bytes = 0;
    int cls, patch_w, pos, pre_g, pre_b, post_g, post_b;
    int64_t wpatch, wpatch3 = -1;
    std::vector<LayerP> layers;
    int T, G, Kpatch, Kraw;
    // the size of the call (GgClipCfg.input_h / input_w; include/gg_clip_interp.h): G x G is the grid of the position TABLE (image_size), Gh x Gw the grid of the
    // input, T = Gh * Gw + 1.  interp: the two differ -- the table is resampled into the weight cache at wpos (T x D f32, the LAST region of the cache)
    int H = 0, W = 0, Gh = 0, Gw = 0; bool interp = false; int64_t wpos = -1;
    // the text tower (gg_clip_text_*) is the same layer stack over T = the call's token count with causal attention: embeddings and the final norm differ
    bool causal = false; int tok_emb = -1, fin_g = -1, fin_b = -1, vocab = 0;
    bool f32, f16, split, fp8 = false; int es;      // fp8: the fp16 mode (f16 is set too) with the encoder Linears as e4m3 products; f32: f32 storage (fp32 and fp32_split modes); split: fp32_split; activation / cached-weight element size: 4 or 2 (bf16 / fp16 modes)
};
static int addt(CModel& m, const std::string& n, std::initializer_list<int64_t> shape) {
    TInfo t; t.name = n; t.ndim = (int)shape.size(); t.numel = 1;
    for (int j = 0; j < 4; ++j) t.shape[j] = 1;
    int i = 0;
    for (auto s : shape) { t.shape[i++] = s; t.numel *= s; }
    t.offset = m.floats; m.floats += gg_align(t.numel, 8);
    m.t.push_back(t);
    return (int)m.t.size() - 1;
}
static int64_t wca(CModel& m, int64_t bytes) { int64_t o = m.wc_bytes; m.wc_bytes += gg_align(bytes, 256); return o; }

// the encoder layers' tensors (HF state-dict order) and their weight-cache images: shared by the vision and the text tower
static void add_layers(CModel& m) {
    const int D = m.cfg.hidden_size, I = m.cfg.intermediate_size;
    auto planes = [&](int64_t n) { return m.split ? wca(m, 3 * n * 2) : (int64_t)-1; };      // fp32_split: bf16 planes [3][n] of a cached matrix
    m.layers.resize(m.cfg.num_layers);
    for (int i = 0; i < m.cfg.num_layers; ++i) {
        LayerP& l = m.layers[i];
        const std::string p = "encoder.layers." + std::to_string(i);
        l.k_w = addt(m, p + ".self_attn.k_proj.weight", {D, D}); l.k_b = addt(m, p + ".self_attn.k_proj.bias", {D});
        l.v_w = addt(m, p + ".self_attn.v_proj.weight", {D, D}); l.v_b = addt(m, p + ".self_attn.v_proj.bias", {D});
        l.q_w = addt(m, p + ".self_attn.q_proj.weight", {D, D}); l.q_b = addt(m, p + ".self_attn.q_proj.bias", {D});
        l.o_w = addt(m, p + ".self_attn.out_proj.weight", {D, D}); l.o_b = addt(m, p + ".self_attn.out_proj.bias", {D});
        l.ln1_g = addt(m, p + ".layer_norm1.weight", {D}); l.ln1_b = addt(m, p + ".layer_norm1.bias", {D});
        l.fc1_w = addt(m, p + ".mlp.fc1.weight", {I, D}); l.fc1_b = addt(m, p + ".mlp.fc1.bias", {I});
        l.fc2_w = addt(m, p + ".mlp.fc2.weight", {D, I}); l.fc2_b = addt(m, p + ".mlp.fc2.bias", {D});
        l.ln2_g = addt(m, p + ".layer_norm2.weight", {D}); l.ln2_b = addt(m, p + ".layer_norm2.bias", {D});
        // W[N][K] for the forward GEMM and W^T[K][N] so that the data gradient dX = dY . W is the same NT GEMM
        l.wqkv = wca(m, (int64_t)3 * D * D * m.es); l.wqkvT = wca(m, (int64_t)3 * D * D * m.es);
        l.bqkv = wca(m, (int64_t)3 * D * 4);
        l.wo = wca(m, (int64_t)D * D * m.es); l.woT = wca(m, (int64_t)D * D * m.es);
        l.w1 = wca(m, (int64_t)I * D * m.es); l.w1T = wca(m, (int64_t)I * D * m.es);
        l.w2 = wca(m, (int64_t)D * I * m.es); l.w2T = wca(m, (int64_t)D * I * m.es);
        l.wqkv3 = planes((int64_t)3 * D * D); l.wqkvT3 = planes((int64_t)3 * D * D); l.wo3 = planes((int64_t)D * D); l.woT3 = planes((int64_t)D * D);
        l.w13 = planes((int64_t)I * D); l.w1T3 = planes((int64_t)I * D); l.w23 = planes((int64_t)D * I); l.w2T3 = planes((int64_t)D * I);
        if (m.fp8) {      // (beside the fp16 images: the mode keeps mode 2's cache layout and adds to it)
            l.wqkv8 = wca(m, (int64_t)3 * D * D); l.wo8 = wca(m, (int64_t)D * D); l.w18 = wca(m, (int64_t)I * D); l.w28 = wca(m, (int64_t)D * I);
            l.sqkv = wca(m, (int64_t)3 * D * 4); l.so = wca(m, (int64_t)D * 4); l.s1 = wca(m, (int64_t)I * 4); l.s2 = wca(m, (int64_t)D * 4);
        }
    }
}

static int build(const GgClipCfg* c, CModel& m) {
    GG_CHECK(c, "clip: null config");
    m.cfg = *c;
    GG_CHECK((c->act_dtype >= 0 && c->act_dtype <= 3) || c->act_dtype == GG_CLIP_ACT_FP8, "clip: act_dtype must be 0 (bf16), 1 (fp32), 2 (fp16), 3 (fp32_split) or 8 (fp8: include/gg_fp8.h), got %d", c->act_dtype);
    m.split = c->act_dtype == 3; m.f32 = c->act_dtype == 1 || m.split; m.fp8 = c->act_dtype == GG_CLIP_ACT_FP8; m.f16 = c->act_dtype == 2 || m.fp8; m.es = m.f32 ? 4 : 2;
    const int D = c->hidden_size, I = c->intermediate_size, P = c->patch_size;
    GG_CHECK(!m.fp8 || (D % 128 == 0 && I % 128 == 0), "clip: the fp8 mode needs hidden_size and intermediate_size multiples of 128 (one K = 128 e4m3 MFMA per stage), got %d / %d", D, I);
    GG_CHECK(D > 0 && D % 64 == 0 && D <= 1024 && c->num_heads > 0 && D / c->num_heads == 64, "clip: head_dim must be 64 and hidden <= 1024 (hidden %d, heads %d)", D, c->num_heads);
    GG_CHECK(P > 0 && c->image_size % P == 0 && I % 8 == 0 && c->num_layers > 0, "clip: bad patch/image/intermediate size or layer count");
    // patch-embedding contraction 3*P*P is padded to a multiple of 8 (ViT-L/14: 588 -> 592 zero columns); sequences beyond 256 tokens
    // (ViT-L/14-336: 577, the reference's CLIP_MODEL, config.py:6) run on the online-softmax attention kernels
    GG_CHECK(c->input_h >= 0 && c->input_w >= 0, "clip: input_h / input_w must be 0 (= image_size) or a size in pixels, got %d x %d", c->input_h, c->input_w);
    m.H = c->input_h ? c->input_h : c->image_size; m.W = c->input_w ? c->input_w : c->image_size;
    GG_CHECK(m.H % P == 0 && m.W % P == 0, "clip: input size %d x %d is not a multiple of the patch size %d", m.H, m.W, P);
    m.G = c->image_size / P; m.Gh = m.H / P; m.Gw = m.W / P; m.interp = m.Gh != m.G || m.Gw != m.G;
    // what gg_clip_pos_interp_fwd / _bwd would refuse is refused here, not mid-forward (D % 4 == 0 follows from D % 64 == 0 above)
    GG_CHECK(!m.interp || (m.G >= 1 && m.Gh >= 1 && m.Gw >= 1), "clip: a grid side below 1 (table %d, input %d x %d patches)", m.G, m.Gh, m.Gw);
    GG_CHECK(!m.interp || (m.G <= GG_CLIP_INTERP_MAX_SIDE && m.Gh <= GG_CLIP_INTERP_MAX_SIDE && m.Gw <= GG_CLIP_INTERP_MAX_SIDE),
             "clip: a grid side above the cap of %d patches for a resampled position table (table %d, input %d x %d patches)", GG_CLIP_INTERP_MAX_SIDE, m.G, m.Gh, m.Gw);
    m.T = m.Gh * m.Gw + 1; m.Kraw = 3 * P * P; m.Kpatch = (int)gg_align(m.Kraw, 8);
    m.cls = addt(m, "embeddings.class_embedding", {D});
    m.patch_w = addt(m, "embeddings.patch_embedding.weight", {D, 3, P, P});
    m.pos = addt(m, "embeddings.position_embedding.weight", {m.G * m.G + 1, D});      // image_size shapes the parameter table, whatever the size of the call
    m.pre_g = addt(m, "pre_layrnorm.weight", {D}); m.pre_b = addt(m, "pre_layrnorm.bias", {D});
    m.wpatch = wca(m, (int64_t)D * m.Kpatch * m.es);
    m.wpatch3 = m.split ? wca(m, 3 * (int64_t)D * m.Kpatch * 2) : (int64_t)-1;              // fp32_split: bf16 planes [3][n] of a cached matrix (no W^T of the patch embedding in either mode: the pixels take no gradient)
    add_layers(m);
    m.post_g = addt(m, "post_layernorm.weight", {D}); m.post_b = addt(m, "post_layernorm.bias", {D});
    if (m.interp) m.wpos = wca(m, (int64_t)m.T * D * 4);      // after everything else: the cache of the native size is a prefix of this one
    return 0;
}
// the text tower's model over `tokens` positions per sequence (the tensor table does not depend on it)
static int build_text(const GgClipTextCfg* c, int tokens, CModel& m) {
    GG_CHECK(c, "clip_text: null config");
    GG_CHECK(c->act_dtype == 0 || c->act_dtype == 1 || c->act_dtype == 3, "clip_text: act_dtype must be 0 (bf16), 1 (fp32) or 3 (fp32_split), got %d (fp16 and fp8 are not built for the text tower)", c->act_dtype);
    const int D = c->hidden_size, I = c->intermediate_size;
    GG_CHECK(D > 0 && D % 64 == 0 && D <= 1024 && c->num_heads > 0 && D / c->num_heads == 64 && D % c->num_heads == 0,
             "clip_text: head_dim must be 64 and hidden <= 1024 (hidden %d, heads %d)", D, c->num_heads);
    GG_CHECK(I > 0 && I % 8 == 0 && c->num_layers > 0 && c->vocab_size > 0, "clip_text: bad intermediate size, layer count or vocabulary");
    GG_CHECK(c->max_positions > 0 && c->max_positions <= GG_CLIP_TEXT_MAX_POSITIONS, "clip_text: max_positions must be 1 ... %d, got %d", GG_CLIP_TEXT_MAX_POSITIONS, c->max_positions);
    GG_CHECK(tokens > 0 && tokens <= c->max_positions, "clip_text: %d tokens per sequence, the position table holds %d", tokens, c->max_positions);
    memset(&m.cfg, 0, sizeof(m.cfg));
    m.cfg.hidden_size = D; m.cfg.intermediate_size = I; m.cfg.num_layers = c->num_layers; m.cfg.num_heads = c->num_heads; m.cfg.ln_eps = c->ln_eps;
    m.cfg.act_dtype = c->act_dtype;
    m.split = c->act_dtype == 3; m.f32 = c->act_dtype == 1 || m.split; m.f16 = false; m.es = m.f32 ? 4 : 2;
    m.causal = true; m.vocab = c->vocab_size; m.T = tokens; m.G = 0; m.Kraw = m.Kpatch = 0;
    m.cls = m.patch_w = m.pre_g = m.pre_b = m.post_g = m.post_b = -1; m.wpatch = -1;
    m.tok_emb = addt(m, "embeddings.token_embedding.weight", {c->vocab_size, D});
    m.pos = addt(m, "embeddings.position_embedding.weight", {c->max_positions, D});
    add_layers(m);
    m.fin_g = addt(m, "final_layer_norm.weight", {D}); m.fin_b = addt(m, "final_layer_norm.bias", {D});
    return 0;
}

// ---- element-type helpers (the storage types of the runtime) -------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ T from_f(float v);
template <> __device__ __forceinline__ float from_f<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16 from_f<bf16>(float v) { return (bf16)v; }
template <> __device__ __forceinline__ f16 from_f<f16>(float v) { return (f16)v; }
// f32 [R][C] -> fp16 copy [R][ldo] and / or transpose [C][ldt] (weight cache of the fp16 mode; the bf16 twin is gg_cast_transpose_f32)
__global__ __launch_bounds__(256) void cast_transpose_f16_kernel(const float* __restrict__ in, int R, int C, f16* __restrict__ out, int64_t ldo,
                                                                f16* __restrict__ outT, int64_t ldt) {
    __shared__ float tile[64][65];
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        const int r = r0 + i, c = c0 + tx;
        float v = 0.f;
        if (r < R && c < C) {
            v = in[(int64_t)r * C + c];
            if (out) out[(int64_t)r * ldo + c] = (f16)v;
        }
        tile[i][tx] = v;
    }
    __syncthreads();
    if (outT) {
        for (int i = ty; i < 64; i += 4) {
            const int c = c0 + i, r = r0 + tx;
            if (c < C && r < R) outT[(int64_t)c * ldt + r] = (f16)tile[tx][i];
        }
    }
}
template <typename TI, typename TO>
__global__ void cast_kernel(const TI* __restrict__ in, TO* __restrict__ out, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = (TO)(float)in[i];
}

// x f32 NCHW (B,3,H,W) -> col [B*Gh*Gw, K], k = (c, py, px)  (== Conv2d(kernel=stride=P) weight flatten); K = 3*P*P padded to 8 (zero columns)
// VEC (P % 8 == 0, W % 4 == 0, 16-byte aligned x): a thread's 8 consecutive k are 8 consecutive pixels of one image row -- two 16-byte loads, one 16-byte
// store, the (c, py, px) split done once per thread instead of once per element (the scalar form ran at 2.5 TB/s on the batch-1024 ViT-B/32 input)
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ x, T* __restrict__ col, int B, int H, int W, int P, int Gh, int Gw, int K) {
    const int Kraw = 3 * P * P;
    const int64_t total = (int64_t)B * Gh * Gw * (K / 8);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int kc = (int)(i % (K / 8)) * 8;
        const int64_t p = i / (K / 8);
        const int gx = (int)(p % Gw), gy = (int)((p / Gw) % Gh), b = (int)(p / ((int64_t)Gh * Gw));
        T o[8];
        if (VEC) {
            if (kc < Kraw) {
                const int c = kc / (P * P), r = kc - c * P * P, py = r / P, px = r - py * P;
                const float* src = x + (((int64_t)b * 3 + c) * H + gy * P + py) * W + gx * P + px;
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) { o[j] = from_f<T>(v0[j]); o[4 + j] = from_f<T>(v1[j]); }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = from_f<T>(0.f);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = kc + j;
                const int c = k / (P * P), py = (k / P) % P, px = k % P;
                o[j] = from_f<T>(k < Kraw ? x[(((int64_t)b * 3 + c) * H + gy * P + py) * W + gx * P + px] : 0.f);
            }
        }
        T* dst = col + p * K + kc;
        if (VEC && sizeof(T) == 2) {
            typedef T t8 __attribute__((ext_vector_type(8)));
            t8 w;
#pragma unroll
            for (int j = 0; j < 8; ++j) w[j] = o[j];
            *reinterpret_cast<t8*>(dst) = w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) dst[j] = o[j];
        }
    }
}
// tokens[b,0,:] = cls + pos[0];  tokens[b,1+i,:] = patches[b,i,:] + pos[1+i]; a thread owns 4 consecutive channels (D % 4 == 0)
template <typename T>
__global__ __launch_bounds__(256) void assemble_tokens_kernel(const T* __restrict__ patches, const float* __restrict__ cls, const float* __restrict__ pos,
                                                              T* __restrict__ tokens, int B, int Tn, int D) {
    const int D4 = D / 4;
    const int64_t total = (int64_t)B * Tn * D4;
    typedef T t4 __attribute__((ext_vector_type(4)));
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int dd = (int)(i % D4) * 4;
        const int64_t bt = i / D4;
        const int t = (int)(bt % Tn);
        const int64_t b = bt / Tn;
        const f32x4 ps = *reinterpret_cast<const f32x4*>(pos + (int64_t)t * D + dd);
        f32x4 v;
        if (t == 0) v = *reinterpret_cast<const f32x4*>(cls + dd);
        else {
            const t4 q = *reinterpret_cast<const t4*>(patches + (b * (Tn - 1) + (t - 1)) * D + dd);
            v = (f32x4){(float)q[0], (float)q[1], (float)q[2], (float)q[3]};
        }
        v += ps;
        t4 w;
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = from_f<T>(v[j]);
        *reinterpret_cast<t4*>(tokens + bt * D + dd) = w;
    }
}
// f32 [R][K] -> T [R][Kp] with zero padding columns
template <typename T>
__global__ void cast_pad_rows_kernel(const float* __restrict__ src, T* __restrict__ dst, int R, int K, int Kp) {
    const int64_t n = (int64_t)R * Kp;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(i % Kp);
        dst[i] = from_f<T>(k < K ? src[(i / Kp) * K + k] : 0.f);
    }
}
// gradient of the token mean (+ an optional gradient on last_hidden_state itself): dx[b,t,:] = dpool[b,:] / T + dlast[b,t,:]
template <typename T>
__global__ void pool_bwd_kernel(const float* __restrict__ dpool, const float* __restrict__ dlast, T* __restrict__ dx, int B, int Tn, int D) {
    const int64_t total = (int64_t)B * Tn * D;
    const float inv = 1.0f / (float)Tn;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int dd = (int)(i % D);
        const int64_t b = i / ((int64_t)D * Tn);
        float v = dpool ? dpool[b * D + dd] * inv : 0.f;
        if (dlast) v += dlast[i];
        dx[i] = from_f<T>(v);
    }
}
// backward of assemble_tokens: dpos[t,:] += sum_b dtok[b,t,:], dcls += sum_b dtok[b,0,:], dpatch[b,i,:] = dtok[b,1+i,:] (contiguous rows for the
// patch-weight gradient GEMM).  One thread per (t, d) column walks the batch: the sums are deterministic.
template <typename T>
__global__ void embed_bwd_kernel(const T* __restrict__ dtok, float* __restrict__ dpos, float* __restrict__ dcls, T* __restrict__ dpatch, int B,
                                 int Tn, int D) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Tn * D) return;
    const int dd = i % D, t = i / D;
    float s = 0.f;
    for (int b = 0; b < B; ++b) {
        const T v = dtok[((int64_t)b * Tn + t) * D + dd];
        s += (float)v;
        if (t > 0 && dpatch) dpatch[((int64_t)b * (Tn - 1) + (t - 1)) * D + dd] = v;
    }
    if (dpos) dpos[i] += s;
    if (t == 0 && dcls) dcls[dd] += s;
}
// dW_patch (D, 3, P, P) += reduced partials [D][Kpatch] (drops the zero-padding columns)
__global__ void patch_wgrad_scatter_kernel(const float* __restrict__ src, int D, int Kp, int Kraw, float* __restrict__ grad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D * Kraw) return;
    grad[i] += src[(int64_t)(i / Kraw) * Kp + i % Kraw];
}
__global__ void copy_f32_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
static inline unsigned grid1d(int64_t n) { return (unsigned)std::min<int64_t>(gg_cdiv(n, 256), 32768); }

// ---- which layers keep their activations ----------------------------------------------------------------------------------------------------------
struct Train {
    bool embed;      // any embedding-side tensor trainable: the backward pass runs through every layer and the patch / position embeddings
    int l0;          // first layer whose activations are kept (num_layers: none)
};
static int first_trained_layer(const CModel& m, const uint8_t* mask) {
    auto on = [&](int t) { return mask == nullptr || mask[t] != 0; };
    for (int i = 0; i < m.cfg.num_layers; ++i) {
        const LayerP& l = m.layers[i];
        const int ids[] = {l.q_w, l.q_b, l.k_w, l.k_b, l.v_w, l.v_b, l.o_w, l.o_b, l.ln1_g, l.ln1_b, l.fc1_w, l.fc1_b, l.fc2_w, l.fc2_b, l.ln2_g, l.ln2_b};
        for (int t : ids) if (on(t)) return i;
    }
    return m.cfg.num_layers;
}
static Train train_of(const CModel& m, int training, const uint8_t* mask) {
    Train tr{false, m.cfg.num_layers};
    if (!training) return tr;
    auto on = [&](int t) { return mask == nullptr || mask[t] != 0; };
    tr.embed = on(m.cls) || on(m.patch_w) || on(m.pos) || on(m.pre_g) || on(m.pre_b);
    tr.l0 = tr.embed ? 0 : first_trained_layer(m, mask);
    return tr;
}

// ---- workspace plan ---------------------------------------------------------------------------------------------------------------------------
struct LayerA { int64_t xin, a1, qkv, o, lse, xmid, a2, pre, h, mean1, rstd1, mean2, rstd2; };
struct CPlan {
    int64_t col, patches, tok, mean0, rstd0;                  // embedding side (tok = tokens before pre_layrnorm)
    int64_t s_x, s_a, s_qkv, s_o, s_h;                        // scratch of the layers that keep nothing (in-place residual stream)
    int64_t q8 = -1, qs = -1;                                 // fp8: the e4m3 codes of the Linear input at hand (M x max(D, I) bytes, reused) and its scale row
    std::vector<LayerA> la;
    int64_t xfinal;
    int64_t dpos_r = -1;                                      // resampled position table (CModel.interp) with a trainable table: embed_bwd's (T, D) f32 sums, which gg_clip_pos_interp_bwd adds into the table's gradient
    int64_t g_x0, g_x1, g_a, g_qkv, g_o, g_h, splitk, colsum, lnscr, lndump, attn_ds = -1;      // lndump: where a frozen LayerNorm tensor's half of a (gamma, beta) gradient pair goes      // backward scratch (attn_ds: GgAttnArgs.ds_scratch)
    int64_t total;
    bool rc = false;                                          // checkpointed layout: every la[i] of a kept layer names the shared segment region but .xin
};
// ds_force: whether attn_ds exists is taken from the recompute-off plan of the same (batch, mask) (1 / 0; -1: decided here) -- its test depends on
// the planned size, and both settings must take the same route through the attention backward
// attention arguments of one layer on B sequences (forward fields; the backward adds its own)
static void clip_attn_args(const CModel& m, int B, GgAttnArgs& at, const void* qkv, void* out, float* lse) {
    const int D = m.cfg.hidden_size;
    memset(&at, 0, sizeof(at));
    at.qkv = qkv; at.ld = 3 * D; at.q_off = 0; at.k_off = D; at.v_off = 2 * D; at.head_stride = 64; at.head_dim = 64;
    at.num_heads = m.cfg.num_heads; at.num_windows = B; at.tokens_per_window = m.T; at.window_size = 0;
    at.scale = 0.125f; at.out = out; at.ldo = D; at.lse = lse;
}
// The ONE place that picks the attention entry point (GG_ATTN_ENTRY_*) and dtype code of a layer: the forward, the backward and the attn_ds plan all ask it,
// and gg_attention_route then says what that entry runs.  Backward: the text tower's causal entry; the opt-in 16-bit-MFMA pair (the dS region is not read);
// else the flash backward.  Forward: the fp8 mode's fp16 attention; the text tower; split products at every token count; the opt-in 16-bit-MFMA forward --
// the training step's kept layers (with lse) and the layers below them alike, the inference forward where nothing is kept --; fp16 MFMA for towers of at most
// 256 tokens (ViT-B/32: 50; beyond: fp16 storage, f32 arithmetic -- gg_attention_fwd_f16 forwards those itself); the flash forward for f32 storage, for kept
// layers (lse) and beyond 256 tokens; else the register-resident forward.
struct AttnCall { int entry, dtype; };
static AttnCall clip_attn_call(bool bwd, bool causal, bool split, bool f32, bool f16, bool fp8, bool attn16, bool attn16t, bool sv, int T) {
    const int dt = split ? 3 : f32 ? 1 : 0;
    if (bwd) return causal ? AttnCall{GG_ATTN_ENTRY_CAUSAL_BWD, dt} : attn16t ? AttnCall{GG_ATTN_ENTRY_FLASH16_BWD, 0} : AttnCall{GG_ATTN_ENTRY_FLASH_BWD, dt};
    if (fp8) return attn16 ? AttnCall{GG_ATTN_ENTRY_FLASH16_FWD, 2} : AttnCall{GG_ATTN_ENTRY_FWD_F16, 0};
    if (causal) return {GG_ATTN_ENTRY_CAUSAL_FWD, dt};
    if (split) return {GG_ATTN_ENTRY_FLASH_FWD, 3};
    if (attn16t) return {GG_ATTN_ENTRY_FLASH16_FWD, 0};
    if (attn16 && !sv) return {GG_ATTN_ENTRY_FLASH16_FWD, f16 ? 2 : 0};
    if (f16) return {GG_ATTN_ENTRY_FWD_F16, 0};
    if (f32 || sv || T > 256) return {GG_ATTN_ENTRY_FLASH_FWD, dt};
    return {GG_ATTN_ENTRY_FWD, 0};
}
static int clip_attn_launch(const AttnCall& c, const GgAttnArgs& at, hipStream_t st) {
    switch (c.entry) {
        case GG_ATTN_ENTRY_CAUSAL_FWD: return gg_attention_causal_fwd(&at, c.dtype, st);
        case GG_ATTN_ENTRY_CAUSAL_BWD: return gg_attention_causal_bwd(&at, c.dtype, st);
        case GG_ATTN_ENTRY_FLASH16_FWD: return gg_attention_flash16_fwd(&at, c.dtype, st);
        case GG_ATTN_ENTRY_FLASH16_BWD: return gg_attention_flash16_bwd(&at, c.dtype, st);
        case GG_ATTN_ENTRY_FLASH_FWD: return gg_attention_flash_fwd(&at, c.dtype, st);
        case GG_ATTN_ENTRY_FLASH_BWD: return gg_attention_flash_bwd(&at, c.dtype, st);
        case GG_ATTN_ENTRY_FWD_F16: return gg_attention_fwd_f16(&at, st);
        default: return gg_attention_fwd(&at, st);
    }
}
static void plan(const CModel& m, int B, const Train& tr, bool training, CPlan& L, int ds_force = -1) {
    const int D = m.cfg.hidden_size, I = m.cfg.intermediate_size, nl = m.cfg.num_layers;
    const int64_t Mp = (int64_t)B * m.Gh * m.Gw, M = (int64_t)B * m.T, es = m.es;
    int64_t off = 0;
    auto al = [&](int64_t bytes) { int64_t o = off; off += gg_align(std::max<int64_t>(bytes, 1), 256); return o; };
    L.col = al(Mp * m.Kpatch * es); L.patches = al(Mp * D * es); L.tok = al(M * D * es); L.mean0 = al(M * 4); L.rstd0 = al(M * 4);
    L.s_x = al(M * D * es); L.s_a = al(M * D * es); L.s_qkv = al(M * 3 * D * es); L.s_o = al(M * D * es); L.s_h = al(M * I * es);
    if (m.fp8) { L.q8 = al(M * std::max(D, I)); L.qs = al(M * 4); }
    L.la.assign(nl, LayerA{});
    L.xfinal = L.s_x;
    const bool bwd = training && tr.l0 < nl;
    L.rc = bwd && m.cfg.recompute != 0;
    if (L.rc && ds_force < 0) {
        CModel m0 = m; m0.cfg.recompute = 0;
        CPlan L0; plan(m0, B, tr, training, L0);
        ds_force = L0.attn_ds >= 0;
    }
    if (bwd) {
        auto inner = [&](LayerA& a) {
            a.a1 = al(M * D * es); a.qkv = al(M * 3 * D * es); a.o = al(M * D * es);
            a.lse = al(M * m.cfg.num_heads * 4); a.xmid = al(M * D * es); a.a2 = al(M * D * es); a.pre = al(M * I * es); a.h = al(M * I * es);
            a.mean1 = al(M * 4); a.rstd1 = al(M * 4); a.mean2 = al(M * 4); a.rstd2 = al(M * 4);
        };
        if (!L.rc) {
            for (int i = tr.l0; i < nl; ++i) { L.la[i].xin = al(M * D * es); inner(L.la[i]); }
            L.xfinal = al(M * D * es);
        } else {
            for (int i = tr.l0; i < nl; ++i) L.la[i].xin = al(M * D * es);
            L.xfinal = al(M * D * es);
            LayerA seg{};
            inner(seg);                                        // the segment region: one layer's worth, re-formed per layer by the backward
            for (int i = tr.l0; i < nl; ++i) { seg.xin = L.la[i].xin; L.la[i] = seg; }
        }
        L.g_x0 = al(M * D * es); L.g_x1 = al(M * D * es); L.g_a = al(M * D * es); L.g_qkv = al(M * 3 * D * es); L.g_o = al(M * D * es);
        L.g_h = al(M * I * es);
        auto splits = [&](int64_t Mm, int N, int K) {
            return (int64_t)(m.split ? gg_gemm_tn_split3_splits((int)Mm, N, K) : m.f32 ? gg_gemm_tn_f32_splits((int)Mm, N, K) : gg_gemm_tn_splits((int)Mm, N, K)) * N * K;
        };
        int64_t sk = std::max(std::max(splits(M, D, I), splits(M, I, D)), splits(M, D, D));
        if (tr.embed && !m.causal) sk = std::max(sk, splits(Mp, D, m.Kpatch));
        L.splitk = al(sk * 4);
        L.colsum = al(std::max(gg_colsum_scratch_floats((int)M, I), gg_colsum_scratch_floats((int)M, D)) * 4);
        L.lnscr = al(gg_layernorm_bwd_scratch_floats(M, D) * 4);
        L.lndump = al((int64_t)D * 4);
        // dS hand-off between the two passes of the attention backward: only towers beyond 256 tokens (ViT-L/14-336: 577 tokens, 22 MB per image) use it -- the
        // 50-token towers run the single-pass kernel --, and only while it stays at most 4 GB and 1/8 of the workspace planned so far
        const int64_t dsb = gg_attention_flash_ds_scratch_floats(B, m.cfg.num_heads, m.T) * 4;
        // the route of the layer's backward when a dS region is given says whether it reads one (placeholder pointers: the report never dereferences them):
        // the fp32_split mode's attention backward recomputes P in both passes (no hand-off at any length), nor does the text tower's causal backward, at most
        // 77 tokens, read one
        GgAttnArgs at;
        GgAttnRoute r;
        void* const given = (void*)(uintptr_t)256;
        clip_attn_args(m, B, at, given, given, (float*)given);
        at.dout = given; at.lddo = D; at.dqkv = given; at.ds_scratch = (float*)given;
        const AttnCall call = clip_attn_call(true, m.causal, m.split, m.f32, m.f16, m.fp8, false, false, true, m.T);
        const bool reads = gg_attention_route(&at, call.entry, call.dtype, &r) == 0 && r.reads_ds_scratch;
        const bool ds = !reads ? false : ds_force >= 0 ? ds_force != 0 : !attn_switches().no_ds_scratch && dsb <= ((int64_t)4 << 30) && dsb <= off / 8;
        if (ds) L.attn_ds = al(dsb);
        if (m.interp && tr.embed && !m.causal) L.dpos_r = al((int64_t)m.T * D * 4);      // (after every region of the native plan)
    }
    L.total = off;
}

// ---- one executing call ---------------------------------------------------------------------------------------------------------------------------
struct Exec {
    const CModel* m; const CPlan* L; int B; hipStream_t st;
    const float* params; const char* wc; char* ws; float* grads; const uint8_t* mask;
    bool attn16t = false;     // a training step (gg_clip_forward with training != 0, gg_clip_backward), switch on (gg_clip_set_attention16_train), a bf16 vision tower beyond 256 tokens: attention through gg_attention_flash16_fwd / _bwd (include/gg_attn16b.h)
    bool attn16 = false;      // gg_clip_forward, inference, switch on (gg_clip_set_attention16), a 16-bit vision tower beyond 256 tokens: attention through gg_attention_flash16_fwd
    const float* P(int t) const { return params + m->t[t].offset; }
    float* Gd(int t) const { return grads + m->t[t].offset; }
    bool tr(int t) const { return mask == nullptr || mask[t] != 0; }
    void* A(int64_t o) const { return ws + o; }
    float* F(int64_t o) const { return reinterpret_cast<float*>(ws + o); }
    const void* W(int64_t o) const { return wc + o; }
    const void* W(int64_t o, int64_t o3) const { return wc + (m->split ? o3 : o); }      // a GEMM's weight operand: the cached matrix, or its bf16 planes (fp32_split)
    int gemm(const void* Am, int64_t lda, const void* Bm, int64_t ldb, void* C, int64_t ldc, int64_t Mm, int N, int K, const float* bias, int act = 0,
             void* preact = nullptr, const void* residual = nullptr, const void* dact_preact = nullptr, int dact = 0) const {
        GgGemmArgs g;
        memset(&g, 0, sizeof(g));
        g.A = Am; g.lda = lda; g.B = Bm; g.ldb = ldb; g.C = C; g.ldc = ldc; g.M = (int)Mm; g.N = N; g.K = K;
        g.bias = bias; g.act = act; g.preact = preact; g.residual = residual; g.ldr = ldc; g.dact_preact = dact_preact; g.dact = dact;
        if (m->split) {      // Bm: planes [3][N][ldb]
            GgSplit3Args s;
            memset(&s, 0, sizeof(s));
            s.b_planes = Bm; s.ldb = ldb; s.M = (int)Mm; s.N = N; s.K = K; s.C = (float*)C; s.ldc = ldc; s.bias = bias; s.act = act; s.preact = (float*)preact;
            s.residual = (const float*)residual; s.ldr = ldc; s.dact_preact = (const float*)dact_preact; s.dact = dact;
            return gg_gemm_nt_split3_af32(&s, (const float*)Am, lda, 0, st);
        }
        return m->f32 ? gg_gemm_nt_f32(&g, st) : (m->f16 ? gg_gemm_nt_f16(&g, st) : gg_gemm_nt(&g, st));
    }
    // partials[splits][N][K] of dY^T . X in the mode's weight-gradient form
    int tn(const void* dY, int64_t ldy, const void* X, int64_t ldx, int64_t M, int N, int K, int* splits) const {
        if (m->split) {
            *splits = gg_gemm_tn_split3_splits((int)M, N, K);
            return gg_gemm_tn_split3((const float*)dY, ldy, (const float*)X, ldx, (int)M, N, K, nullptr, 0, F(L->splitk), *splits, st);
        }
        *splits = m->f32 ? gg_gemm_tn_f32_splits((int)M, N, K) : gg_gemm_tn_splits((int)M, N, K);
        if (m->f32) return gg_gemm_tn_f32(dY, ldy, X, ldx, (int)M, N, K, nullptr, 0, F(L->splitk), *splits, st);
        return gg_gemm_tn(dY, ldy, X, ldx, (int)M, N, K, nullptr, 0, F(L->splitk), *splits, st);
    }
    // fp8: C fp16 = epi(sa * sw * (codes of A in L->q8 . W8^T) + bias); the codes and L->qs were left by ln_fwd8 / quant8
    int gemm8(int64_t w8, int64_t sw, void* C, int64_t ldc, int64_t Mm, int N, int K, const float* bias, int act = 0, const void* residual = nullptr) const {
        GgGemmArgs g;
        memset(&g, 0, sizeof(g));
        g.A = A(L->q8); g.lda = K; g.B = W(w8); g.ldb = K; g.C = C; g.ldc = ldc; g.M = (int)Mm; g.N = N; g.K = K;
        g.bias = bias; g.act = act; g.residual = residual; g.ldr = ldc;
        return gg_gemm_nt_e4m3(&g, F(L->qs), (const float*)W(sw), st);
    }
    int quant8(const void* x, int64_t M, int K) const { return gg_quant_rows_e4m3(x, 0, K, M, K, A(L->q8), K, F(L->qs), st); }
    int ln_fwd8(const void* x, int tg, int tb, int64_t M) const {
        return gg_layernorm_fwd_e4m3(x, P(tg), P(tb), M, m->cfg.hidden_size, m->cfg.ln_eps, A(L->q8), m->cfg.hidden_size, F(L->qs), st);
    }
    int ln_fwd(const void* x, int tg, int tb, int64_t M, void* out, float* mean, float* rstd) const {
        if (m->f16) return gg_layernorm_fwd_f16(x, P(tg), P(tb), M, m->cfg.hidden_size, m->cfg.ln_eps, out, st);
        return gg_layernorm_fwd(x, m->f32, P(tg), P(tb), M, m->cfg.hidden_size, m->cfg.ln_eps, out, m->f32, mean, rstd, st);
    }
    // dx = LayerNorm backward of dout (+ dres), dgamma / dbeta accumulated when trainable
    int ln_bwd(const void* dout, const void* x, const float* mean, const float* rstd, int tg, int tb, int64_t M, const void* dres, void* dx) const {
        const bool t = tr(tg) || tr(tb);
        // the kernel forms dgamma and dbeta together: when only one of the two is trainable, the other's sums are added to a dump row nobody reads, never into the frozen
        // tensor's region of the flat gradient buffer (which the caller may be exchanging / reading as zeros)
        return gg_layernorm_bwd(dout, x, m->f32, mean, rstd, P(tg), M, m->cfg.hidden_size, dres, dx, F(L->lnscr), t ? (tr(tg) ? Gd(tg) : F(L->lndump)) : nullptr,
                                t ? (tr(tb) ? Gd(tb) : F(L->lndump)) : nullptr, 1, st);
    }
    // dW[N,K] += dY[M,N]^T . X[M,K]
    int wgrad(int tw, const void* dY, int64_t ldy, const void* X, int64_t ldx, int64_t M, int N, int K) const {
        if (!tr(tw)) return 0;
        int sp;
        GG_TRY(tn(dY, ldy, X, ldx, M, N, K, &sp));
        return gg_splitk_reduce(F(L->splitk), Gd(tw), (int64_t)N * K, sp, 1, 1.0f, st);
    }
    int bgrad(int tb, const void* dY, int64_t ld, int64_t M, int N) const {
        if (!tr(tb)) return 0;
        if (m->f32) return gg_colsum_f32((const float*)dY, ld, (int)M, N, nullptr, 0, F(L->colsum), Gd(tb), 1, st);
        return gg_colsum_bf16(dY, ld, (int)M, N, nullptr, 0, F(L->colsum), Gd(tb), 1, st);
    }
    void attn_args(GgAttnArgs& at, const void* qkv, void* out, float* lse) const { clip_attn_args(*m, B, at, qkv, out, lse); }
    int attention(const GgAttnArgs& at, bool bwd, bool sv) const {
        return clip_attn_launch(clip_attn_call(bwd, m->causal, m->split, m->f32, m->f16, m->fp8, attn16, attn16t, sv, m->T), at, st);
    }
};
template <typename T> static int embed_fwd(const Exec& e, const float* x, void* tok_out) {
    const CModel& m = *e.m; const CPlan& L = *e.L;
    const int D = m.cfg.hidden_size, B = e.B;
    const int64_t Mp = (int64_t)B * m.Gh * m.Gw, M = (int64_t)B * m.T;
    const bool pvec = (m.cfg.patch_size & 7) == 0 && (m.W & 3) == 0 && ((uintptr_t)x & 15) == 0;
    if (pvec) hipLaunchKernelGGL((patchify_kernel<T, true>), dim3(grid1d(Mp * (m.Kpatch / 8))), dim3(256), 0, e.st, x, (T*)e.A(L.col), B, m.H, m.W, m.cfg.patch_size, m.Gh, m.Gw, m.Kpatch);
    else hipLaunchKernelGGL((patchify_kernel<T, false>), dim3(grid1d(Mp * (m.Kpatch / 8))), dim3(256), 0, e.st, x, (T*)e.A(L.col), B, m.H, m.W, m.cfg.patch_size, m.Gh, m.Gw, m.Kpatch);
    GG_LAUNCH_CHECK();
    GG_TRY(e.gemm(e.A(L.col), m.Kpatch, e.W(m.wpatch, m.wpatch3), m.Kpatch, e.A(L.patches), D, Mp, D, m.Kpatch, nullptr));
    hipLaunchKernelGGL(assemble_tokens_kernel<T>, dim3(grid1d(M * D / 4)), dim3(256), 0, e.st, (const T*)e.A(L.patches), e.P(m.cls), m.interp ? (const float*)e.W(m.wpos) : e.P(m.pos), (T*)tok_out,
                       B, m.T, D);
    GG_LAUNCH_CHECK();
    return 0;
}
// One encoder layer's forward from `cur`: LN1, qkv, attention, out_proj + residual, LN2, fc1 with QuickGELU (+ the pre-activation when kept), and
// fc2 + residual into `next` (next < 0: skipped -- the recompute of a kept layer, whose fc2 output is the next layer's kept input).  sv: the layer's
// tensors are kept in L.la[i] for its backward.  gg_clip_forward and the recompute of gg_clip_backward both come through here: same entry points,
// same arguments.
static int layer_fwd(const Exec& e, int i, int64_t cur, int64_t next, bool sv) {
    const CModel& m = *e.m; const CPlan& L = *e.L;
    const LayerP& l = m.layers[i];
    const LayerA& a = L.la[i];
    const int D = m.cfg.hidden_size, I = m.cfg.intermediate_size, T = m.T;
    const int64_t M = (int64_t)e.B * T;
    const int64_t A1 = sv ? a.a1 : L.s_a, QKV = sv ? a.qkv : L.s_qkv, O = sv ? a.o : L.s_o, XMID = sv ? a.xmid : cur, A2 = sv ? a.a2 : L.s_a,
                  H = sv ? a.h : L.s_h;
    if (m.fp8) {
        // mode 2's layer with each Linear's input as e4m3 codes + row scales in L.q8 / L.qs (one buffer: every Linear consumes its input before the next is formed)
        GG_CHECK(!sv && next >= 0, "clip: the fp8 mode is inference-only");
        GG_TRY(e.ln_fwd8(e.A(cur), l.ln1_g, l.ln1_b, M));
        GG_TRY(e.gemm8(l.wqkv8, l.sqkv, e.A(QKV), 3 * D, M, 3 * D, D, (const float*)e.W(l.bqkv)));
        GgAttnArgs at8;
        e.attn_args(at8, e.A(QKV), e.A(O), nullptr);
        GG_TRY(e.attention(at8, false, sv));
        GG_TRY(e.quant8(e.A(O), M, D));
        GG_TRY(e.gemm8(l.wo8, l.so, e.A(XMID), D, M, D, D, e.P(l.o_b), 0, e.A(cur)));
        GG_TRY(e.ln_fwd8(e.A(XMID), l.ln2_g, l.ln2_b, M));
        GG_TRY(e.gemm8(l.w18, l.s1, e.A(H), I, M, I, D, e.P(l.fc1_b), GG_ACT_CODE_QUICK_GELU));
        GG_TRY(e.quant8(e.A(H), M, I));
        GG_TRY(e.gemm8(l.w28, l.s2, e.A(next), D, M, D, I, e.P(l.fc2_b), 0, e.A(XMID)));
        return 0;
    }
    GG_TRY(e.ln_fwd(e.A(cur), l.ln1_g, l.ln1_b, M, e.A(A1), sv ? e.F(a.mean1) : nullptr, sv ? e.F(a.rstd1) : nullptr));
    GG_TRY(e.gemm(e.A(A1), D, e.W(l.wqkv, l.wqkv3), D, e.A(QKV), 3 * D, M, 3 * D, D, (const float*)e.W(l.bqkv)));
    GgAttnArgs at;
    e.attn_args(at, e.A(QKV), e.A(O), sv ? e.F(a.lse) : nullptr);
    GG_TRY(e.attention(at, false, sv));
    // x_mid = x + out_proj(o)   (in place when nothing is kept: each element is read then written by the same lane)
    GG_TRY(e.gemm(e.A(O), D, e.W(l.wo, l.wo3), D, e.A(XMID), D, M, D, D, e.P(l.o_b), 0, nullptr, e.A(cur)));
    GG_TRY(e.ln_fwd(e.A(XMID), l.ln2_g, l.ln2_b, M, e.A(A2), sv ? e.F(a.mean2) : nullptr, sv ? e.F(a.rstd2) : nullptr));
    if (m.causal && !m.f32 && sv) {
        // bf16 text tower, kept layer: the bf16 GEMM's pre-activation epilogue applies QuickGELU to the ROUNDED pre-activation, the inference epilogue to the f32
        // accumulator.  The training forward must give the inference forward's bits, so fc1 runs the inference epilogue, and a second, linear pass leaves the copy
        GG_TRY(e.gemm(e.A(A2), D, e.W(l.w1, l.w13), D, e.A(H), I, M, I, D, e.P(l.fc1_b), GG_ACT_CODE_QUICK_GELU, nullptr));
        GG_TRY(e.gemm(e.A(A2), D, e.W(l.w1, l.w13), D, e.A(a.pre), I, M, I, D, e.P(l.fc1_b)));
    } else
    GG_TRY(e.gemm(e.A(A2), D, e.W(l.w1, l.w13), D, e.A(H), I, M, I, D, e.P(l.fc1_b), GG_ACT_CODE_QUICK_GELU, sv ? e.A(a.pre) : nullptr));
    if (next >= 0) GG_TRY(e.gemm(e.A(H), I, e.W(l.w2, l.w23), I, e.A(next), D, M, D, I, e.P(l.fc2_b), 0, nullptr, e.A(XMID)));
    return 0;
}

// The backward of the encoder layers nl - 1 .. l0 (gg_clip_backward and gg_clip_text_backward both come through here).  In: `dx` holds the gradient of the top
// layer's output; out: `dx` names the region with the gradient of layer l0's input (dx / other swap between L.g_x0 and L.g_x1).  The towers differ in the
// attention backward only (causal for the text tower).
static int layers_bwd(const Exec& e, int l0, bool top_in_region, int64_t& dx, int64_t& other) {
    const CModel& m = *e.m; const CPlan& L = *e.L;
    const int D = m.cfg.hidden_size, I = m.cfg.intermediate_size, nl = m.cfg.num_layers;
    const int64_t M = (int64_t)e.B * m.T;
    for (int i = nl - 1; i >= l0; --i) {
        const LayerP& l = m.layers[i];
        const LayerA& a = L.la[i];
        // activation recompute: the layer's tensors are re-formed in the segment region from its kept input (the top layer's are still the forward's in the first
        // backward after it)
        if (L.rc && (i < nl - 1 || !top_in_region)) GG_TRY(layer_fwd(e, i, a.xin, -1, true));
        // ---- MLP: x_out = x_mid + fc2(quick_gelu(fc1(LN2(x_mid))))
        GG_TRY(e.wgrad(l.fc2_w, e.A(dx), D, e.A(a.h), I, M, D, I));
        GG_TRY(e.bgrad(l.fc2_b, e.A(dx), D, M, D));
        GG_TRY(e.gemm(e.A(dx), D, e.W(l.w2T, l.w2T3), D, e.A(L.g_h), I, M, I, D, nullptr, 0, nullptr, nullptr, e.A(a.pre), GG_ACT_CODE_QUICK_GELU));   // d pre
        GG_TRY(e.wgrad(l.fc1_w, e.A(L.g_h), I, e.A(a.a2), D, M, I, D));
        GG_TRY(e.bgrad(l.fc1_b, e.A(L.g_h), I, M, I));
        GG_TRY(e.gemm(e.A(L.g_h), I, e.W(l.w1T, l.w1T3), I, e.A(L.g_a), D, M, D, I, nullptr));                                                        // d LN2 out
        GG_TRY(e.ln_bwd(e.A(L.g_a), e.A(a.xmid), e.F(a.mean2), e.F(a.rstd2), l.ln2_g, l.ln2_b, M, e.A(dx), e.A(other)));                       // d x_mid
        std::swap(dx, other);
        // ---- attention: x_mid = x_in + out_proj(attn(qkv(LN1(x_in))))
        GG_TRY(e.wgrad(l.o_w, e.A(dx), D, e.A(a.o), D, M, D, D));
        GG_TRY(e.bgrad(l.o_b, e.A(dx), D, M, D));
        GG_TRY(e.gemm(e.A(dx), D, e.W(l.woT, l.woT3), D, e.A(L.g_o), D, M, D, D, nullptr));                                                            // d o
        GgAttnArgs at;
        e.attn_args(at, e.A(a.qkv), e.A(a.o), e.F(a.lse));
        at.dout = e.A(L.g_o); at.lddo = D; at.dqkv = e.A(L.g_qkv);
        if (L.attn_ds >= 0) at.ds_scratch = e.F(L.attn_ds);
        GG_TRY(e.attention(at, true, true));
        const char* dq = (const char*)e.A(L.g_qkv);
        GG_TRY(e.wgrad(l.q_w, dq, 3 * D, e.A(a.a1), D, M, D, D));
        GG_TRY(e.wgrad(l.k_w, dq + (int64_t)D * m.es, 3 * D, e.A(a.a1), D, M, D, D));
        GG_TRY(e.wgrad(l.v_w, dq + (int64_t)2 * D * m.es, 3 * D, e.A(a.a1), D, M, D, D));
        GG_TRY(e.bgrad(l.q_b, dq, 3 * D, M, D));
        GG_TRY(e.bgrad(l.k_b, dq + (int64_t)D * m.es, 3 * D, M, D));
        GG_TRY(e.bgrad(l.v_b, dq + (int64_t)2 * D * m.es, 3 * D, M, D));
        GG_TRY(e.gemm(e.A(L.g_qkv), 3 * D, e.W(l.wqkvT, l.wqkvT3), 3 * D, e.A(L.g_a), D, M, D, 3 * D, nullptr));                                          // d LN1 out
        GG_TRY(e.ln_bwd(e.A(L.g_a), e.A(a.xin), e.F(a.mean1), e.F(a.rstd1), l.ln1_g, l.ln1_b, M, e.A(dx), e.A(other)));                         // d x_in
        std::swap(dx, other);
    }
    return 0;
}

// What the library has seen happen to a training workspace, by its address (host side): WS_RC -- the training forward that last wrote it ran the
// checkpointed layout; WS_TOP -- the segment region still holds that forward's top layer (no backward has re-formed a lower layer in it since).
// gg_clip_backward refuses the other layout, whose offsets name other bytes, and skips the top layer's recompute only while WS_TOP stands; a
// workspace it knows nothing of (-1) is neither refused nor trusted: every layer is re-formed.  So the table only ever saves work or adds a
// refusal, results never depend on it.  It is process-global state in an otherwise stateless API, bounded by dropping everything at 4096
// entries; keys outlive the allocations they named (a freed and reused address keeps its entry until the next training forward there rewrites
// it -- a backward is only defined after such a forward).
enum { WS_RC = 1, WS_TOP = 2 };
static std::mutex g_ws_mu;
static std::map<const void*, int> g_ws_state;
static void ws_forget(const void* ws) {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    g_ws_state.erase(ws);
}
static void ws_note(const void* ws, int state) {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    if (g_ws_state.size() >= 4096 && !g_ws_state.count(ws)) g_ws_state.clear();
    g_ws_state[ws] = state;
}
static int ws_state(const void* ws) {      // -1: unknown
    std::lock_guard<std::mutex> lk(g_ws_mu);
    auto it = g_ws_state.find(ws);
    return it == g_ws_state.end() ? -1 : it->second;
}
static void ws_clear_top(const void* ws) {      // (an unknown workspace stays unknown)
    std::lock_guard<std::mutex> lk(g_ws_mu);
    auto it = g_ws_state.find(ws);
    if (it != g_ws_state.end()) it->second &= ~WS_TOP;
}
}  // namespace

extern "C" int gg_cast_f32_to_f16(const float* in, void* out, int64_t n, void* stream) {
    GG_CHECK(in && out && n > 0, "gg_cast_f32_to_f16: bad args");
    hipLaunchKernelGGL((cast_kernel<float, f16>), dim3(grid1d(n)), dim3(256), 0, (hipStream_t)stream, in, (f16*)out, n);
    GG_LAUNCH_CHECK();
    return 0;
}
extern "C" int gg_cast_f16_to_f32(const void* in, float* out, int64_t n, void* stream) {
    GG_CHECK(in && out && n > 0, "gg_cast_f16_to_f32: bad args");
    hipLaunchKernelGGL((cast_kernel<f16, float>), dim3(grid1d(n)), dim3(256), 0, (hipStream_t)stream, (const f16*)in, out, n);
    GG_LAUNCH_CHECK();
    return 0;
}
extern "C" int gg_clip_num_tensors(const GgClipCfg* cfg) { CModel m; return build(cfg, m) ? -1 : (int)m.t.size(); }
extern "C" int gg_clip_tensor_info(const GgClipCfg* cfg, int i, char* name, int cap, int64_t* offset, int64_t* numel, int* ndim, int64_t* shape4) {
    CModel m;
    GG_TRY(build(cfg, m));
    GG_CHECK(i >= 0 && i < (int)m.t.size(), "gg_clip_tensor_info: index out of range");
    if (name && cap > 0) snprintf(name, cap, "%s", m.t[i].name.c_str());
    if (offset) *offset = m.t[i].offset;
    if (numel) *numel = m.t[i].numel;
    if (ndim) *ndim = m.t[i].ndim;
    if (shape4) for (int j = 0; j < 4; ++j) shape4[j] = m.t[i].shape[j];
    return 0;
}
extern "C" int64_t gg_clip_param_floats(const GgClipCfg* cfg) { CModel m; return build(cfg, m) ? -1 : m.floats; }
extern "C" int64_t gg_clip_wcache_bytes(const GgClipCfg* cfg) { CModel m; return build(cfg, m) ? -1 : m.wc_bytes; }
extern "C" int64_t gg_clip_workspace_bytes(const GgClipCfg* cfg, int batch, int training, const uint8_t* trainable) {
    CModel m;
    if (build(cfg, m)) return -1;
    if (batch <= 0) { gg_set_error("gg_clip_workspace_bytes: batch must be > 0"); return -1; }
    CPlan L; plan(m, batch, train_of(m, training, trainable), training != 0, L);
    return L.total;
}
extern "C" int gg_clip_first_trained_layer(const GgClipCfg* cfg, const uint8_t* trainable) {
    CModel m;
    if (build(cfg, m)) return -1;
    return train_of(m, 1, trainable).l0;
}
static int refresh_model(const CModel& m, const float* params, void* wcache, const uint8_t* only, void* stream);
extern "C" int gg_clip_refresh_weights(const GgClipCfg* cfg, const float* params, void* wcache, void* stream) {
    CModel m;
    GG_TRY(build(cfg, m));
    return refresh_model(m, params, wcache, nullptr, stream);
}
// `only` (host, one byte per tensor, or NULL = every tensor): the tensors whose cached forms -- copy, transpose and, in the fp32_split mode, the bf16 planes of both --
// are rebuilt.  The public entry point rebuilds everything; a masked one (the per-step refresh of a last-layer fine-tune skipping every frozen layer) needs only an export.
// (the text tower comes through here too: it has no patch embedding)
static int refresh_model(const CModel& m, const float* params, void* wcache, const uint8_t* only, void* stream) {
    GG_CHECK(params && wcache, "gg_clip_refresh_weights: null pointer");
    GG_CHECK(!m.interp || (((uintptr_t)params & 15) == 0 && ((uintptr_t)wcache & 15) == 0), "gg_clip_refresh_weights: a resampled position table needs 16-byte aligned params and wcache");
    char* wc = (char*)wcache;
    hipStream_t st = (hipStream_t)stream;
    const int D = m.cfg.hidden_size, I = m.cfg.intermediate_size;
    auto P = [&](int t) { return params + m.t[t].offset; };
    // W f32 [R][C] -> cache copy [R][C] at `n` (row offset r0 of a taller [.., C] image) and transpose [C][ldt] at `t` (column offset c0)
    auto ch = [&](int t) { return only == nullptr || only[t] != 0; };
    // planes of a cached f32 matrix [R][C] (fp32_split; the matrix was just rebuilt)
    auto split3 = [&](int64_t src, int64_t R, int C, int64_t dst) -> int {
        return m.split ? gg_split3_bf16((const float*)(wc + src), R, C, C, wc + dst, st) : 0;
    };
    auto put = [&](int tw, int R, int C, int64_t n, int64_t r0, int64_t t, int64_t ldt, int64_t c0) -> int {
        if (!ch(tw)) return 0;
        const float* W = P(tw);
        if (m.f32) {
            GG_HIP(hipMemcpyAsync(wc + n + r0 * C * 4, W, (size_t)R * C * 4, hipMemcpyDeviceToDevice, st));
            return gg_transpose_f32(W, R, C, (float*)(wc + t) + c0, ldt, st);
        }
        if (m.f16) {
            hipLaunchKernelGGL(cast_transpose_f16_kernel, dim3((unsigned)gg_cdiv(C, 64), (unsigned)gg_cdiv(R, 64)), dim3(256), 0, st, W, R, C,
                               (f16*)(wc + n) + r0 * C, (int64_t)C, (f16*)(wc + t) + c0, ldt);
            GG_LAUNCH_CHECK();
            return 0;
        }
        return gg_cast_transpose_f32(W, R, C, (bf16*)(wc + n) + r0 * C, C, (bf16*)(wc + t) + c0, ldt, st);
    };
    if (m.causal || !ch(m.patch_w)) {}
    else if (m.f16) hipLaunchKernelGGL(cast_pad_rows_kernel<f16>, dim3(grid1d((int64_t)D * m.Kpatch)), dim3(256), 0, st, P(m.patch_w), (f16*)(wc + m.wpatch), D, m.Kraw, m.Kpatch);
    else if (m.f32) hipLaunchKernelGGL(cast_pad_rows_kernel<float>, dim3(grid1d((int64_t)D * m.Kpatch)), dim3(256), 0, st, P(m.patch_w), (float*)(wc + m.wpatch), D, m.Kraw, m.Kpatch);
    else hipLaunchKernelGGL(cast_pad_rows_kernel<bf16>, dim3(grid1d((int64_t)D * m.Kpatch)), dim3(256), 0, st, P(m.patch_w), (bf16*)(wc + m.wpatch), D, m.Kraw, m.Kpatch);
    GG_LAUNCH_CHECK();
    if (!m.causal && ch(m.patch_w)) GG_TRY(split3(m.wpatch, D, m.Kpatch, m.wpatch3));
    if (m.interp && ch(m.pos)) GG_TRY(gg_clip_pos_interp_fwd(P(m.pos), m.G, m.Gh, m.Gw, D, (float*)(wc + m.wpos), stream));      // the table at the size of the call
    for (auto& l : m.layers) {
        GG_TRY(put(l.q_w, D, D, l.wqkv, 0, l.wqkvT, 3 * D, 0));
        GG_TRY(put(l.k_w, D, D, l.wqkv, D, l.wqkvT, 3 * D, D));
        GG_TRY(put(l.v_w, D, D, l.wqkv, 2 * D, l.wqkvT, 3 * D, 2 * D));
        if (ch(l.q_w) || ch(l.k_w) || ch(l.v_w)) {      // (the three projections share one [3D][D] image)
            GG_TRY(split3(l.wqkv, 3 * D, D, l.wqkv3));
            GG_TRY(split3(l.wqkvT, D, 3 * D, l.wqkvT3));
        }
        float* bq = (float*)(wc + l.bqkv);
        if (ch(l.q_b)) hipLaunchKernelGGL(copy_f32_kernel, dim3((unsigned)gg_cdiv(D, 256)), dim3(256), 0, st, P(l.q_b), bq, D);
        if (ch(l.k_b)) hipLaunchKernelGGL(copy_f32_kernel, dim3((unsigned)gg_cdiv(D, 256)), dim3(256), 0, st, P(l.k_b), bq + D, D);
        if (ch(l.v_b)) hipLaunchKernelGGL(copy_f32_kernel, dim3((unsigned)gg_cdiv(D, 256)), dim3(256), 0, st, P(l.v_b), bq + 2 * D, D);
        GG_TRY(put(l.o_w, D, D, l.wo, 0, l.woT, D, 0));
        GG_TRY(put(l.fc1_w, I, D, l.w1, 0, l.w1T, I, 0));
        GG_TRY(put(l.fc2_w, D, I, l.w2, 0, l.w2T, D, 0));
        if (ch(l.o_w)) { GG_TRY(split3(l.wo, D, D, l.wo3)); GG_TRY(split3(l.woT, D, D, l.woT3)); }
        if (ch(l.fc1_w)) { GG_TRY(split3(l.w1, I, D, l.w13)); GG_TRY(split3(l.w1T, D, I, l.w1T3)); }
        if (ch(l.fc2_w)) { GG_TRY(split3(l.w2, D, I, l.w23)); GG_TRY(split3(l.w2T, I, D, l.w2T3)); }
        if (m.fp8) {      // e4m3 images from the f32 master weights, one scale per output channel (the three projections are rows of one image)
            auto q8 = [&](int tw, int64_t R, int C, int64_t img, int64_t sc, int64_t r0) -> int {
                return ch(tw) ? gg_quant_rows_e4m3(P(tw), 1, C, R, C, wc + img + r0 * C, C, (float*)(wc + sc) + r0, st) : 0;
            };
            GG_TRY(q8(l.q_w, D, D, l.wqkv8, l.sqkv, 0)); GG_TRY(q8(l.k_w, D, D, l.wqkv8, l.sqkv, D)); GG_TRY(q8(l.v_w, D, D, l.wqkv8, l.sqkv, 2 * D));
            GG_TRY(q8(l.o_w, D, D, l.wo8, l.so, 0)); GG_TRY(q8(l.fc1_w, I, D, l.w18, l.s1, 0)); GG_TRY(q8(l.fc2_w, D, I, l.w28, l.s2, 0));
        }
    }
    GG_LAUNCH_CHECK();
    return 0;
}

// the opt-in long-row attention of the inference forward (include/gg_attn16.h); process-wide like tinyvit.hip's g_drop_compact
static std::atomic<int> g_attention16{0};
extern "C" int gg_clip_set_attention16(int on) { return g_attention16.exchange(on != 0 ? 1 : 0); }
// the same for the training step (include/gg_attn16b.h): a switch of its own, read when gg_clip_forward(training) or gg_clip_backward is enqueued
static std::atomic<int> g_attention16_train{0};
extern "C" int gg_clip_set_attention16_train(int on) { return g_attention16_train.exchange(on != 0 ? 1 : 0); }
static bool attention16_train_route(const CModel& m) {
    return g_attention16_train.load() != 0 && !m.causal && !m.f32 && !m.f16 && !m.fp8 && m.T > 256;      // bf16 (act_dtype 0) vision towers beyond 256 tokens
}

extern "C" int gg_clip_forward(const GgClipCfg* cfg, int batch, int training, const float* params, const void* wcache, const float* x, void* workspace,
                               float* out, float* last_hidden, const uint8_t* trainable, void* stream) {
    CModel m;
    GG_TRY(build(cfg, m));
    GG_CHECK(batch > 0 && params && wcache && x && workspace && out, "gg_clip_forward: null pointer / bad batch");
    GG_CHECK(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)wcache & 255) == 0, "gg_clip_forward: workspace / wcache must be 256-byte aligned");
    const Train tr = train_of(m, training, trainable);
    GG_CHECK(!(m.fp8 && training), "gg_clip_forward: the fp8 mode is inference-only (training = 1 refused; train in fp32 or bf16)");
    GG_CHECK(!(m.f16 && training && tr.l0 < m.cfg.num_layers), "gg_clip_forward: the fp16 mode is inference-only (train in fp32 or bf16)");
    CPlan L; plan(m, batch, tr, training != 0, L);
    Exec e{&m, &L, batch, (hipStream_t)stream, params, (const char*)wcache, (char*)workspace, nullptr, trainable};
    e.attn16t = training != 0 && attention16_train_route(m);
    e.attn16 = !training && g_attention16.load() != 0 && !m.causal && !m.f32 && m.T > 256;      // (m.f32 covers fp32 and fp32_split; fp8 is an fp16 mode)
    const int D = m.cfg.hidden_size, T = m.T, B = batch, nl = m.cfg.num_layers;
    const int64_t M = (int64_t)B * T;
    const bool keep = training && tr.l0 < nl;
    if (keep) ws_forget(workspace);                 // until every launch below is enqueued, the workspace holds no forward the table could vouch for
    auto saved = [&](int i) { return keep && i >= tr.l0; };
    GG_TRY(m.f32 ? embed_fwd<float>(e, x, e.A(L.tok)) : (m.f16 ? embed_fwd<f16>(e, x, e.A(L.tok)) : embed_fwd<bf16>(e, x, e.A(L.tok))));
    int64_t cur = saved(0) ? L.la[0].xin : L.s_x;
    GG_TRY(e.ln_fwd(e.A(L.tok), m.pre_g, m.pre_b, M, e.A(cur), keep && tr.embed ? e.F(L.mean0) : nullptr, keep && tr.embed ? e.F(L.rstd0) : nullptr));
    for (int i = 0; i < nl; ++i) {
        const int64_t next = (keep && i + 1 >= tr.l0) ? (i + 1 < nl ? L.la[i + 1].xin : L.xfinal) : cur;
        GG_TRY(layer_fwd(e, i, cur, next, saved(i)));
        cur = next;
    }
    if (m.f32) {
        GG_TRY(gg_token_mean_fwd_f32((const float*)e.A(cur), out, B, T, D, e.st));
        if (last_hidden) GG_HIP(hipMemcpyAsync(last_hidden, e.A(cur), (size_t)M * D * 4, hipMemcpyDeviceToDevice, e.st));
    } else if (m.f16) {
        GG_TRY(gg_token_mean_fwd_f16(e.A(cur), out, B, T, D, e.st));
        if (last_hidden) GG_TRY(gg_cast_f16_to_f32(e.A(cur), last_hidden, M * D, e.st));
    } else {
        GG_TRY(gg_token_mean_fwd(e.A(cur), out, B, T, D, e.st));
        if (last_hidden) GG_TRY(gg_cast_bf16_to_f32(e.A(cur), last_hidden, M * D, e.st));
    }
    if (keep) ws_note(workspace, (L.rc ? WS_RC : 0) | WS_TOP);
    return 0;
}

// Backward of the training forward that last wrote `workspace` (same cfg, batch and trainable mask).  d_out: gradient of the pooled mean
// (batch, hidden) or NULL; d_last_hidden: gradient of last_hidden_state (batch, T, hidden) or NULL (both given: summed).  Gradients of the
// trainable tensors are ACCUMULATED into `grads` (flat, same offsets as params); post_layernorm is not on the path (its gradient is zero).
extern "C" int gg_clip_backward(const GgClipCfg* cfg, int batch, const float* params, const void* wcache, void* workspace, const float* d_out,
                                const float* d_last_hidden, float* grads, const uint8_t* trainable, void* stream) {
    CModel m;
    GG_TRY(build(cfg, m));
    GG_CHECK(batch > 0 && params && wcache && workspace && grads && (d_out || d_last_hidden), "gg_clip_backward: null pointer / bad batch");
    GG_CHECK(!m.fp8, "gg_clip_backward: the fp8 mode is inference-only");
    GG_CHECK(!m.interp || (((uintptr_t)grads & 15) == 0 && ((uintptr_t)workspace & 15) == 0), "gg_clip_backward: a resampled position table needs 16-byte aligned grads and workspace");
    const Train tr = train_of(m, 1, trainable);
    const int nl = m.cfg.num_layers;
    if (tr.l0 >= nl) return 0;                    // nothing in the tower is trainable
    GG_CHECK(!m.f16, "gg_clip_backward: the fp16 mode is inference-only");
    CPlan L; plan(m, batch, tr, true, L);
    const int seen = ws_state(workspace);
    GG_CHECK(seen < 0 || ((seen & WS_RC) != 0) == L.rc, "gg_clip_backward: cfg->recompute = %d, but the forward that last wrote this workspace ran with recompute = %d "
             "(the checkpointed layout keeps other tensors); run the forward again", L.rc ? 1 : 0, seen & WS_RC);
    // The top layer is the one layer whose tensors the forward leaves in the segment region.  Re-forming a lower layer overwrites them, so a further backward of
    // the same forward (retain_graph, d_out and d_last_hidden in two calls) re-forms the top layer as well -- as does a backward that cannot tell.
    const bool top_in_region = seen >= 0 && (seen & WS_TOP) != 0;
    if (L.rc && tr.l0 < nl - 1) ws_clear_top(workspace);
    Exec e{&m, &L, batch, (hipStream_t)stream, params, (const char*)wcache, (char*)workspace, grads, trainable};
    e.attn16t = attention16_train_route(m);       // the recompute replay and the attention backward
    const int D = m.cfg.hidden_size, I = m.cfg.intermediate_size, T = m.T, B = batch;
    const int64_t M = (int64_t)B * T, Mp = (int64_t)B * m.Gh * m.Gw;
    if (m.f32) hipLaunchKernelGGL(pool_bwd_kernel<float>, dim3(grid1d(M * D)), dim3(256), 0, e.st, d_out, d_last_hidden, (float*)e.A(L.g_x0), B, T, D);
    else hipLaunchKernelGGL(pool_bwd_kernel<bf16>, dim3(grid1d(M * D)), dim3(256), 0, e.st, d_out, d_last_hidden, (bf16*)e.A(L.g_x0), B, T, D);
    GG_LAUNCH_CHECK();
    int64_t dx = L.g_x0, other = L.g_x1;
    GG_TRY(layers_bwd(e, tr.l0, top_in_region, dx, other));
    if (!tr.embed) return 0;
    // ---- embeddings: x_0 = pre_layrnorm(tokens), tokens = [cls ; patches . W^T] + pos
    GG_TRY(e.ln_bwd(e.A(dx), e.A(L.tok), e.F(L.mean0), e.F(L.rstd0), m.pre_g, m.pre_b, M, nullptr, e.A(other)));
    const bool wp = e.tr(m.patch_w);
    // a resampled table: the sums over the batch are the gradient of the (T, D) table the forward read; its adjoint resampling adds them into the parameter's
    const bool rpos = m.interp && e.tr(m.pos);
    if (rpos) GG_HIP(hipMemsetAsync(e.A(L.dpos_r), 0, (size_t)T * D * 4, e.st));
    float* dpos = rpos ? e.F(L.dpos_r) : e.tr(m.pos) ? e.Gd(m.pos) : nullptr;
    float* dcls = e.tr(m.cls) ? e.Gd(m.cls) : nullptr;
    if (m.f32) hipLaunchKernelGGL(embed_bwd_kernel<float>, dim3((unsigned)gg_cdiv((int64_t)T * D, 256)), dim3(256), 0, e.st, (const float*)e.A(other), dpos, dcls,
                                  wp ? (float*)e.A(L.g_a) : nullptr, B, T, D);
    else hipLaunchKernelGGL(embed_bwd_kernel<bf16>, dim3((unsigned)gg_cdiv((int64_t)T * D, 256)), dim3(256), 0, e.st, (const bf16*)e.A(other), dpos, dcls,
                            wp ? (bf16*)e.A(L.g_a) : nullptr, B, T, D);
    GG_LAUNCH_CHECK();
    if (rpos) GG_TRY(gg_clip_pos_interp_bwd(e.F(L.dpos_r), m.G, m.Gh, m.Gw, D, e.Gd(m.pos), e.st));
    if (wp) {
        int sp;
        GG_TRY(e.tn(e.A(L.g_a), D, e.A(L.col), m.Kpatch, Mp, D, m.Kpatch, &sp));
        GG_TRY(gg_splitk_reduce(e.F(L.splitk), e.F(L.splitk), (int64_t)D * m.Kpatch, sp, 0, 1.0f, e.st));
        hipLaunchKernelGGL(patch_wgrad_scatter_kernel, dim3((unsigned)gg_cdiv((int64_t)D * m.Kraw, 256)), dim3(256), 0, e.st, e.F(L.splitk), D, m.Kpatch,
                           m.Kraw, e.Gd(m.patch_w));
        GG_LAUNCH_CHECK();
    }
    return 0;
}

// ================================================================== CLIP text tower (include/gg_clip_text.h): forward for frozen weights
// transformers CLIPTextModel as pretrain_idun.py:205-300 runs it inside CLIPModel.forward: token + position embedding, the encoder layers above with the causal
// attention, final_layer_norm, the row at the EOS position.  Inference schedule only: the residual stream and the layer temporaries recycle five regions.
namespace {
// tokens[b,t,:] = token_embedding[id[b,t]] + position_embedding[t]; a lane owns 4 consecutive channels (one 16-byte load of each table).  An id outside
// [0, vocab) is clamped: the Python layer refuses such input, the kernel must not read outside the table either way.
template <typename T>
__global__ __launch_bounds__(256) void text_embed_kernel(const int32_t* __restrict__ ids, const float* __restrict__ tok, const float* __restrict__ pos,
                                                         T* __restrict__ out, int64_t rows, int Tn, int D, int vocab) {
    const int D4 = D / 4;
    const int64_t total = rows * D4;
    typedef T t4 __attribute__((ext_vector_type(4)));
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int dd = (int)(i % D4) * 4;
        const int64_t bt = i / D4;
        const int t = (int)(bt % Tn);
        const int id = min(max(ids[bt], 0), vocab - 1);
        const f32x4 v = *reinterpret_cast<const f32x4*>(tok + (int64_t)id * D + dd) + *reinterpret_cast<const f32x4*>(pos + (int64_t)t * D + dd);
        t4 w;
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = from_f<T>(v[j]);
        *reinterpret_cast<t4*>(out + bt * D + dd) = w;
    }
}
// pooled[b,:] = x[b, pos[b], :] (GATHER) / dx[b,t,:] = t == pos[b] ? dpooled[b,:] : 0 (the backward: every element of dx is written)
template <bool GATHER>
__global__ __launch_bounds__(256) void row_pick_kernel(const float* __restrict__ src, const int32_t* __restrict__ pos, float* __restrict__ dst, int B, int Tn, int C) {
    const int C4 = C / 4;
    const int64_t total = GATHER ? (int64_t)B * C4 : (int64_t)B * Tn * C4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int dd = (int)(i % C4) * 4;
        const int64_t r = i / C4;
        if (GATHER) {
            const int t = pos ? min(max(pos[r], 0), Tn - 1) : 0;
            *reinterpret_cast<f32x4*>(dst + r * C + dd) = *reinterpret_cast<const f32x4*>(src + (r * Tn + t) * C + dd);
        } else {
            const int64_t b = r / Tn;
            const int t = (int)(r % Tn), tp = pos ? min(max(pos[b], 0), Tn - 1) : 0;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (t == tp) v = *reinterpret_cast<const f32x4*>(src + b * C + dd);
            *reinterpret_cast<f32x4*>(dst + r * C + dd) = v;
        }
    }
}
struct TextPlan : CPlan { int64_t fin; };
static void plan_text(const CModel& m, int B, TextPlan& L) {
    const int D = m.cfg.hidden_size, I = m.cfg.intermediate_size;
    const int64_t M = (int64_t)B * m.T, es = m.es;
    int64_t off = 0;
    auto al = [&](int64_t bytes) { int64_t o = off; off += gg_align(std::max<int64_t>(bytes, 1), 256); return o; };
    L.s_x = al(M * D * es); L.s_a = al(M * D * es); L.s_qkv = al(M * 3 * D * es); L.s_o = al(M * D * es); L.s_h = al(M * I * es);
    L.fin = al(M * D * 4);                                    // final_layer_norm's f32 rows when the caller does not take last_hidden
    L.la.assign(m.cfg.num_layers, LayerA{});
    L.xfinal = L.s_x;
    L.total = off;
}
}  // namespace

extern "C" int gg_row_gather_f32(const float* x, const int32_t* pos, float* pooled, int B, int T, int C, void* stream) {
    GG_CHECK(x && pooled && B > 0 && T > 0 && C > 0 && (C & 3) == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)pooled & 15) == 0, "gg_row_gather_f32: bad args (C %% 4, 16-byte alignment)");
    GG_PROF(GG_CAT_MOVE, 0, 8.0 * B * C, stream);
    hipLaunchKernelGGL(row_pick_kernel<true>, dim3(grid1d((int64_t)B * C / 4)), dim3(256), 0, (hipStream_t)stream, x, pos, pooled, B, T, C);
    GG_LAUNCH_CHECK();
    return 0;
}
extern "C" int gg_row_scatter_f32(const float* dpooled, const int32_t* pos, float* dx, int B, int T, int C, void* stream) {
    GG_CHECK(dpooled && dx && B > 0 && T > 0 && C > 0 && (C & 3) == 0 && ((uintptr_t)dx & 15) == 0 && ((uintptr_t)dpooled & 15) == 0, "gg_row_scatter_f32: bad args (C %% 4, 16-byte alignment)");
    GG_PROF(GG_CAT_MOVE, 0, 4.0 * B * T * C, stream);
    hipLaunchKernelGGL(row_pick_kernel<false>, dim3(grid1d((int64_t)B * T * C / 4)), dim3(256), 0, (hipStream_t)stream, dpooled, pos, dx, B, T, C);
    GG_LAUNCH_CHECK();
    return 0;
}
extern "C" int gg_clip_text_num_tensors(const GgClipTextCfg* cfg) { CModel m; return build_text(cfg, 1, m) ? -1 : (int)m.t.size(); }
extern "C" int gg_clip_text_tensor_info(const GgClipTextCfg* cfg, int i, char* name, int cap, int64_t* offset, int64_t* numel, int* ndim, int64_t* shape4) {
    CModel m;
    GG_TRY(build_text(cfg, 1, m));
    GG_CHECK(i >= 0 && i < (int)m.t.size(), "gg_clip_text_tensor_info: index out of range");
    if (name && cap > 0) snprintf(name, cap, "%s", m.t[i].name.c_str());
    if (offset) *offset = m.t[i].offset;
    if (numel) *numel = m.t[i].numel;
    if (ndim) *ndim = m.t[i].ndim;
    if (shape4) for (int j = 0; j < 4; ++j) shape4[j] = m.t[i].shape[j];
    return 0;
}
extern "C" int64_t gg_clip_text_param_floats(const GgClipTextCfg* cfg) { CModel m; return build_text(cfg, 1, m) ? -1 : m.floats; }
extern "C" int64_t gg_clip_text_wcache_bytes(const GgClipTextCfg* cfg) { CModel m; return build_text(cfg, 1, m) ? -1 : m.wc_bytes; }
extern "C" int64_t gg_clip_text_workspace_bytes(const GgClipTextCfg* cfg, int batch, int tokens) {
    CModel m;
    if (build_text(cfg, tokens, m)) return -1;
    if (batch <= 0) { gg_set_error("gg_clip_text_workspace_bytes: batch must be > 0"); return -1; }
    TextPlan L; plan_text(m, batch, L);
    return L.total;
}
extern "C" int gg_clip_text_refresh_weights(const GgClipTextCfg* cfg, const float* params, void* wcache, void* stream) {
    CModel m;
    GG_TRY(build_text(cfg, 1, m));
    return refresh_model(m, params, wcache, nullptr, stream);
}
extern "C" int gg_clip_text_forward(const GgClipTextCfg* cfg, int batch, int tokens, const float* params, const void* wcache, const int32_t* input_ids,
                                    const int32_t* eos_pos, void* workspace, float* last_hidden, float* pooled, void* stream) {
    CModel m;
    GG_TRY(build_text(cfg, tokens, m));
    GG_CHECK(batch > 0 && params && wcache && input_ids && eos_pos && workspace && pooled, "gg_clip_text_forward: null pointer / bad batch");
    GG_CHECK(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)wcache & 255) == 0, "gg_clip_text_forward: workspace / wcache must be 256-byte aligned");
    GG_CHECK(((uintptr_t)pooled & 15) == 0 && ((uintptr_t)last_hidden & 15) == 0 && ((uintptr_t)params & 15) == 0, "gg_clip_text_forward: params / last_hidden / pooled must be 16-byte aligned");
    TextPlan L; plan_text(m, batch, L);
    Exec e{&m, &L, batch, (hipStream_t)stream, params, (const char*)wcache, (char*)workspace, nullptr, nullptr};
    const int D = m.cfg.hidden_size, T = m.T;
    const int64_t M = (int64_t)batch * T;
    {      // (a scope of its own: the profiler times a scope, and the launches below carry their own)
    GG_PROF(GG_CAT_MOVE, 0, (4.0 + m.es) * M * D, stream);
    if (m.f32) hipLaunchKernelGGL(text_embed_kernel<float>, dim3(grid1d(M * D / 4)), dim3(256), 0, e.st, input_ids, e.P(m.tok_emb), e.P(m.pos), (float*)e.A(L.s_x), M, T, D, m.vocab);
    else hipLaunchKernelGGL(text_embed_kernel<bf16>, dim3(grid1d(M * D / 4)), dim3(256), 0, e.st, input_ids, e.P(m.tok_emb), e.P(m.pos), (bf16*)e.A(L.s_x), M, T, D, m.vocab);
    GG_LAUNCH_CHECK();
    }
    for (int i = 0; i < m.cfg.num_layers; ++i) GG_TRY(layer_fwd(e, i, L.s_x, L.s_x, false));      // in place, as the vision tower's inference layers
    float* fin = last_hidden ? last_hidden : e.F(L.fin);
    GG_TRY(gg_layernorm_fwd(e.A(L.s_x), m.f32, e.P(m.fin_g), e.P(m.fin_b), M, D, m.cfg.ln_eps, fin, 1, nullptr, nullptr, e.st));
    return gg_row_gather_f32(fin, eos_pos, pooled, batch, T, D, e.st);
}

// ================================================================== CLIP text tower, training (include/gg_clip_text_train.h)
// The vision tower's machinery over the text model: plan / LayerA keep the tensors of the layers from the first trained one up, layer_fwd(sv = true) fills them,
// layers_bwd walks them back with the causal attention backward.  Around it: the head (d_pooled scattered to the EOS rows + d_last_hidden, final_layer_norm's
// backward) and the tail (token-embedding scatter-add, position sum).  No activation recompute.
namespace {
struct TextTrain { bool any, embed, fin; int l0; };      // anything trainable; an embedding table; final_layer_norm; first kept layer
static TextTrain text_train_of(const CModel& m, const uint8_t* mask) {
    auto on = [&](int t) { return mask == nullptr || mask[t] != 0; };
    TextTrain tt;
    tt.embed = on(m.tok_emb) || on(m.pos);
    tt.fin = on(m.fin_g) || on(m.fin_b);
    tt.l0 = tt.embed ? 0 : first_trained_layer(m, mask);
    tt.any = tt.embed || tt.fin || tt.l0 < m.cfg.num_layers;
    return tt;
}
struct TextTrainPlan : CPlan { int64_t fin, fmean, frstd, dx32 = -1; };
// plan()'s layout (its embedding-side regions are empty here) + final_layer_norm's output and statistics; with no layer kept, the few regions its backward needs
static void plan_text_train(const CModel& m, int B, const TextTrain& tt, TextTrainPlan& L) {
    const int D = m.cfg.hidden_size, nl = m.cfg.num_layers;
    const int64_t M = (int64_t)B * m.T, es = m.es;
    plan(m, B, Train{tt.embed, tt.l0}, true, L);
    int64_t off = L.total;
    auto al = [&](int64_t bytes) { int64_t o = off; off += gg_align(std::max<int64_t>(bytes, 1), 256); return o; };
    L.fin = al(M * D * 4); L.fmean = al(M * 4); L.frstd = al(M * 4);
    if (tt.l0 >= nl) {      // only final_layer_norm trains
        L.g_a = al(M * D * es); L.g_x0 = al(M * D * es);
        L.lnscr = al(gg_layernorm_bwd_scratch_floats(M, D) * 4); L.lndump = al((int64_t)D * 4);
    }
    if (tt.embed && !m.f32) L.dx32 = al(M * D * 4);      // the scatter-add reads f32 rows
    L.total = off;
}
// dy[b,t,:] = (t == eos[b] ? d_pooled[b,:] : 0) + d_last[b,t,:] in the storage type (either source may be NULL); every element of dy is written
template <typename T>
__global__ __launch_bounds__(256) void text_head_bwd_kernel(const float* __restrict__ dpool, const float* __restrict__ dlast, const int32_t* __restrict__ pos,
                                                            T* __restrict__ dy, int B, int Tn, int D) {
    const int D4 = D / 4;
    const int64_t total = (int64_t)B * Tn * D4;
    typedef T t4 __attribute__((ext_vector_type(4)));
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int dd = (int)(i % D4) * 4;
        const int64_t r = i / D4, b = r / Tn;
        const int t = (int)(r % Tn);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (dpool && t == min(max(pos[b], 0), Tn - 1)) v = *reinterpret_cast<const f32x4*>(dpool + b * D + dd);
        if (dlast) v += *reinterpret_cast<const f32x4*>(dlast + r * D + dd);
        t4 w;
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = from_f<T>(v[j]);
        *reinterpret_cast<t4*>(dy + r * D + dd) = w;
    }
}
// scatter-add, pass 1: cid[r] = the clamped id, lead[r] = no earlier row carries it (a wave's lanes walk the earlier rows together: broadcast loads)
__global__ __launch_bounds__(256) void scatter_lead_kernel(const int32_t* __restrict__ ids, int64_t rows, int vocab, int32_t* __restrict__ cid, int32_t* __restrict__ lead) {
    const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const int id = min(max(ids[r], 0), vocab - 1);
    int first = 1;
    for (int64_t q = 0; q < r; ++q)
        if (min(max(ids[q], 0), vocab - 1) == id) { first = 0; break; }
    cid[r] = id;
    lead[r] = first;
}
// pass 2: one workgroup per row; a leader's adds the rows r.. that carry its id, in index order, and then the sum onto the table row.  Rows are matched 256 at a
// time (one per thread, a ballot per wave), then every thread walks the set bits -- the same order in every thread, whatever the launch.
__global__ __launch_bounds__(256) void scatter_add_kernel(const float* __restrict__ dx, const int32_t* __restrict__ cid, const int32_t* __restrict__ lead,
                                                          float* __restrict__ dtable, int64_t rows, int D) {
    __shared__ unsigned long long hit[4];
    const int64_t r = blockIdx.x;
    if (!lead[r]) return;                                          // (workgroup-uniform)
    const int id = cid[r];
    const int D4 = D / 4, wave = threadIdx.x >> 6;
    f32x4 acc[4];                                                  // columns 4 (threadIdx.x + 256 j): D <= 4096
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int64_t r0 = r; r0 < rows; r0 += 256) {
        const int64_t q = r0 + threadIdx.x;
        const unsigned long long b = __ballot(q < rows && cid[q] == id);
        __syncthreads();                                           // the previous chunk's masks have been read
        if ((threadIdx.x & 63) == 0) hit[wave] = b;
        __syncthreads();
        for (int w = 0; w < 4; ++w) {
            unsigned long long mk = hit[w];
            while (mk) {
                const int bit = __builtin_ctzll(mk);
                mk &= mk - 1;
                const float* src = dx + (r0 + 64 * w + bit) * D;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c4 = threadIdx.x + 256 * j;
                    if (c4 < D4) acc[j] += *reinterpret_cast<const f32x4*>(src + 4 * c4);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c4 = threadIdx.x + 256 * j;
        if (c4 < D4) {
            f32x4* dst = reinterpret_cast<f32x4*>(dtable + (int64_t)id * D + 4 * c4);
            *dst = *dst + acc[j];
        }
    }
}
}  // namespace

extern "C" int64_t gg_embedding_scatter_add_scratch_bytes(int64_t rows) {
    if (rows <= 0) { gg_set_error("gg_embedding_scatter_add_scratch_bytes: rows must be > 0"); return -1; }
    return gg_align(rows * 8, 256);                                // int32 cid[rows] | int32 lead[rows]
}
extern "C" int gg_embedding_scatter_add_f32(const float* dx, const int32_t* ids, float* dtable, int64_t rows, int D, int vocab, void* scratch, void* stream) {
    GG_CHECK(dx && ids && dtable && scratch && rows > 0 && rows < ((int64_t)1 << 31) && vocab > 0, "gg_embedding_scatter_add_f32: null pointer / bad row or vocabulary count");
    GG_CHECK(D > 0 && (D & 3) == 0 && D <= 4096, "gg_embedding_scatter_add_f32: D must be a multiple of 4, at most 4096 (got %d)", D);
    GG_CHECK(((uintptr_t)dx & 15) == 0 && ((uintptr_t)dtable & 15) == 0 && ((uintptr_t)scratch & 15) == 0, "gg_embedding_scatter_add_f32: dx / dtable / scratch must be 16-byte aligned");
    int32_t* cid = (int32_t*)scratch;
    int32_t* lead = cid + rows;
    GG_PROF(GG_CAT_MOVE, 0, 4.0 * rows * D * 3, stream);
    hipLaunchKernelGGL(scatter_lead_kernel, dim3((unsigned)gg_cdiv(rows, 256)), dim3(256), 0, (hipStream_t)stream, ids, rows, vocab, cid, lead);
    hipLaunchKernelGGL(scatter_add_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, dx, cid, lead, dtable, rows, D);
    GG_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t gg_clip_text_train_workspace_bytes(const GgClipTextCfg* cfg, int batch, int tokens, const uint8_t* trainable) {
    CModel m;
    if (build_text(cfg, tokens, m)) return -1;
    if (batch <= 0) { gg_set_error("gg_clip_text_train_workspace_bytes: batch must be > 0"); return -1; }
    const TextTrain tt = text_train_of(m, trainable);
    if (!tt.any) { TextPlan L; plan_text(m, batch, L); return L.total; }
    TextTrainPlan L; plan_text_train(m, batch, tt, L);
    return L.total;
}
extern "C" int gg_clip_text_first_trained_layer(const GgClipTextCfg* cfg, const uint8_t* trainable) {
    CModel m;
    if (build_text(cfg, 1, m)) return -1;
    return text_train_of(m, trainable).l0;
}
extern "C" int gg_clip_text_forward_train(const GgClipTextCfg* cfg, int batch, int tokens, const float* params, const void* wcache, const int32_t* input_ids,
                                          const int32_t* eos_pos, void* workspace, float* last_hidden, float* pooled, const uint8_t* trainable, void* stream) {
    CModel m;
    GG_TRY(build_text(cfg, tokens, m));
    const TextTrain tt = text_train_of(m, trainable);
    if (!tt.any) return gg_clip_text_forward(cfg, batch, tokens, params, wcache, input_ids, eos_pos, workspace, last_hidden, pooled, stream);      // nothing is kept
    GG_CHECK(batch > 0 && params && wcache && input_ids && eos_pos && workspace && pooled, "gg_clip_text_forward_train: null pointer / bad batch");
    GG_CHECK(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)wcache & 255) == 0, "gg_clip_text_forward_train: workspace / wcache must be 256-byte aligned");
    GG_CHECK(((uintptr_t)pooled & 15) == 0 && ((uintptr_t)last_hidden & 15) == 0 && ((uintptr_t)params & 15) == 0, "gg_clip_text_forward_train: params / last_hidden / pooled must be 16-byte aligned");
    TextTrainPlan L; plan_text_train(m, batch, tt, L);
    Exec e{&m, &L, batch, (hipStream_t)stream, params, (const char*)wcache, (char*)workspace, nullptr, trainable};
    const int D = m.cfg.hidden_size, T = m.T, nl = m.cfg.num_layers;
    const int64_t M = (int64_t)batch * T;
    const bool keep = tt.l0 < nl;
    auto saved = [&](int i) { return keep && i >= tt.l0; };
    int64_t cur = saved(0) ? L.la[0].xin : L.s_x;
    {
    GG_PROF(GG_CAT_MOVE, 0, (4.0 + m.es) * M * D, stream);
    if (m.f32) hipLaunchKernelGGL(text_embed_kernel<float>, dim3(grid1d(M * D / 4)), dim3(256), 0, e.st, input_ids, e.P(m.tok_emb), e.P(m.pos), (float*)e.A(cur), M, T, D, m.vocab);
    else hipLaunchKernelGGL(text_embed_kernel<bf16>, dim3(grid1d(M * D / 4)), dim3(256), 0, e.st, input_ids, e.P(m.tok_emb), e.P(m.pos), (bf16*)e.A(cur), M, T, D, m.vocab);
    GG_LAUNCH_CHECK();
    }
    for (int i = 0; i < nl; ++i) {
        const int64_t next = (keep && i + 1 >= tt.l0) ? (i + 1 < nl ? L.la[i + 1].xin : L.xfinal) : cur;
        GG_TRY(layer_fwd(e, i, cur, next, saved(i)));
        cur = next;
    }
    float* fin = last_hidden ? last_hidden : e.F(L.fin);
    GG_TRY(gg_layernorm_fwd(e.A(cur), m.f32, e.P(m.fin_g), e.P(m.fin_b), M, D, m.cfg.ln_eps, fin, 1, e.F(L.fmean), e.F(L.frstd), e.st));
    return gg_row_gather_f32(fin, eos_pos, pooled, batch, T, D, e.st);
}
extern "C" int gg_clip_text_backward(const GgClipTextCfg* cfg, int batch, int tokens, const float* params, const void* wcache, const int32_t* input_ids,
                                     const int32_t* eos_pos, void* workspace, const float* d_pooled, const float* d_last_hidden, float* grads,
                                     const uint8_t* trainable, void* stream) {
    CModel m;
    GG_TRY(build_text(cfg, tokens, m));
    const TextTrain tt = text_train_of(m, trainable);
    if (!tt.any) return 0;                          // nothing in the tower is trainable
    GG_CHECK(batch > 0 && params && wcache && workspace && grads && (d_pooled || d_last_hidden), "gg_clip_text_backward: null pointer / bad batch");
    GG_CHECK(!d_pooled || eos_pos, "gg_clip_text_backward: d_pooled needs eos_pos");
    GG_CHECK(!tt.embed || input_ids, "gg_clip_text_backward: a trainable embedding table needs input_ids");
    GG_CHECK(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)wcache & 255) == 0, "gg_clip_text_backward: workspace / wcache must be 256-byte aligned");
    GG_CHECK(((uintptr_t)d_pooled & 15) == 0 && ((uintptr_t)d_last_hidden & 15) == 0 && ((uintptr_t)params & 15) == 0 && ((uintptr_t)grads & 15) == 0,
             "gg_clip_text_backward: params / grads / d_pooled / d_last_hidden must be 16-byte aligned");
    TextTrainPlan L; plan_text_train(m, batch, tt, L);
    Exec e{&m, &L, batch, (hipStream_t)stream, params, (const char*)wcache, (char*)workspace, grads, trainable};
    const int D = m.cfg.hidden_size, T = m.T, B = batch, nl = m.cfg.num_layers;
    const int64_t M = (int64_t)B * T;
    // ---- head: pooled = final_layer_norm(x)[eos]
    {
    GG_PROF(GG_CAT_MOVE, 0, (4.0 + m.es) * M * D, stream);
    if (m.f32) hipLaunchKernelGGL(text_head_bwd_kernel<float>, dim3(grid1d(M * D / 4)), dim3(256), 0, e.st, d_pooled, d_last_hidden, eos_pos, (float*)e.A(L.g_a), B, T, D);
    else hipLaunchKernelGGL(text_head_bwd_kernel<bf16>, dim3(grid1d(M * D / 4)), dim3(256), 0, e.st, d_pooled, d_last_hidden, eos_pos, (bf16*)e.A(L.g_a), B, T, D);
    GG_LAUNCH_CHECK();
    }
    const int64_t xfin = tt.l0 < nl ? L.xfinal : L.s_x;
    GG_TRY(e.ln_bwd(e.A(L.g_a), e.A(xfin), e.F(L.fmean), e.F(L.frstd), m.fin_g, m.fin_b, M, nullptr, e.A(L.g_x0)));
    if (tt.l0 >= nl) return 0;
    int64_t dx = L.g_x0, other = L.g_x1;
    GG_TRY(layers_bwd(e, tt.l0, true, dx, other));
    if (!tt.embed) return 0;
    // ---- embeddings: x_0[b,t,:] = token_embedding[id[b,t]] + position_embedding[t]
    if (e.tr(m.pos)) {
        GG_PROF(GG_CAT_MOVE, 0, (double)m.es * M * D, stream);
        if (m.f32) hipLaunchKernelGGL(embed_bwd_kernel<float>, dim3((unsigned)gg_cdiv((int64_t)T * D, 256)), dim3(256), 0, e.st, (const float*)e.A(dx), e.Gd(m.pos), (float*)nullptr,
                                      (float*)nullptr, B, T, D);
        else hipLaunchKernelGGL(embed_bwd_kernel<bf16>, dim3((unsigned)gg_cdiv((int64_t)T * D, 256)), dim3(256), 0, e.st, (const bf16*)e.A(dx), e.Gd(m.pos), (float*)nullptr,
                                (bf16*)nullptr, B, T, D);
        GG_LAUNCH_CHECK();
    }
    if (e.tr(m.tok_emb)) {
        const float* dx32 = (const float*)e.A(dx);
        if (!m.f32) { GG_TRY(gg_cast_bf16_to_f32(e.A(dx), e.F(L.dx32), M * D, e.st)); dx32 = e.F(L.dx32); }
        // (the clamped ids and leader flags, 8 bytes a row, go where d attention-output was, at least 128 bytes a row: the layers are done with it)
        GG_TRY(gg_embedding_scatter_add_f32(dx32, input_ids, e.Gd(m.tok_emb), M, D, m.vocab, e.A(L.g_o), e.st));
    }
    return 0;
}
