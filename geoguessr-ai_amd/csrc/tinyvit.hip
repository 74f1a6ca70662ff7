// TinyViT encoder runtime: parameter table, bf16 weight cache, workspace plan, whole-network forward and
// backward as a static schedule of libgg kernels on one HIP stream (no tracing compiler, no per-op host
// round trips).  Architecture: timm TinyVit (TinyViT, Wu et al. 2022) as instantiated by the reference through
// timm.create_model(name, num_classes=0, global_pool="avg") -- models/tinyvit.py:48-53,135; SURVEY.md App. A.
// Activations are NHWC bf16 ([tokens, channels]), so every 1x1 conv / Linear is a plain GEMM and the
// BHWC<->BCHW permutes of TinyVitBlock vanish.
#include <string>
#include <vector>
#include <map>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <atomic>
#include "common.h"
#include "graph.h"
#include "../../include/gg.h"
#include "../../include/gg_cls.h"
#include "../../include/gg_drop.h"
#include "../../include/gg_pad.h"
#include "../../include/gg_attn16w.h"
#include "../../include/gg_attn16wb.h"
#include "../../include/gg_attn_dbias.h"
#include "../../include/gg_wgrad_resident.h"
#include "../../include/gg_conv_dgrad_parity.h"
#include "attention_route.h"

bool gg_split3_af32_takes_rowmap(int N, int K);      // gemm_split3.hip: the form gg_gemm_nt_split3_af32 would run this shape on accepts row compaction

namespace {

// DropPath row compaction of frozen stage-2 blocks (gg_tinyvit_set_drop_compact; block_compacts below)
std::atomic<int> g_drop_compact{1};
// the opt-in 16-bit-MFMA attention of the bf16 inference forward for windows beyond 256 tokens (gg_tinyvit_set_attention16, include/gg_attn16w.h)
std::atomic<int> g_attention16{0};
// the opt-in 16-bit-MFMA attention of the bf16 TRAINING step for windows beyond 256 tokens (gg_tinyvit_set_attention16_train, include/gg_attn16wb.h)
std::atomic<int> g_attention16_train{0};
// the opt-in fixed-order bias gradient of the training step (gg_tinyvit_set_deterministic_dbias, include/gg_attn_dbias.h)
std::atomic<int> g_deterministic_dbias{0};

struct TensorInfo { std::string name; int64_t offset; int64_t numel; int ndim; int64_t shape[4]; int kind; };
static const float kAttnScale = 0.17677669529663687f;   // head_dim 32 ^ -0.5; the expanded bias tables are divided by it
struct DenseW { int t_w = -1, t_b = -1; int N = 0, K = 0, Kp = 0, Np = 0, taps = 1, cin = 0; int64_t wn = 0, wt = 0;
                int64_t wn3 = -1, wt3 = -1; };     // fp32_split mode: bf16 planes [3][N][Kp] / [3][Kp][Np] of the cached f32 W / W^T (gg_gemm_nt_split3's B operand)
struct BNP { int t_g = -1, t_b = -1; int64_t rm = 0, rv = 0; int cnt = 0; int C = 0; };
struct DwW { int t_w = -1; int C = 0; int64_t taps = 0; };
struct LNP { int t_g = -1, t_b = -1; int C = 0; };
struct ConvBNDense { DenseW w; BNP bn; };
struct ConvBNDw { DwW w; BNP bn; };
struct MBConvL { ConvBNDense c1; ConvBNDw c2; ConvBNDense c3; };
struct MergeL { ConvBNDense c1; ConvBNDw c2; ConvBNDense c3; };
struct BlockL { int t_ab = -1; int64_t bias_full = 0; LNP ln1; DenseW qkv, proj; LNP ln2; DenseW fc1, fc2; ConvBNDw local; };
struct StageL { MergeL merge; std::vector<BlockL> blocks; int C, heads, ws, res, pres; };      // pres: the map side the attention branch runs at -- res rounded up to a multiple of ws (timm pads bottom / right)
// The geometry and layout of a stage's window attention on B images.  The pointers a forward needs hold a placeholder (16-byte aligned, never dereferenced):
// gg_attention_route only asks whether a pointer is given and aligned, so the planner and the compaction test ask it about these arguments as they are;
// attn_args overwrites them with the block's tensors.
static void attn_shape(const StageL& st, int B, GgAttnArgs& at) {
    const int C = st.C;
    memset(&at, 0, sizeof(at));
    at.ld = 3 * C; at.q_off = 0; at.k_off = 32; at.v_off = 64; at.head_stride = 96; at.head_dim = 32;
    at.num_heads = st.heads; at.tokens_per_window = st.ws * st.ws;
    at.num_windows = B * (st.pres / st.ws) * (st.pres / st.ws);
    at.window_size = st.ws; at.map_h = st.pres; at.map_w = st.pres;      // (a padded block: the padded map)
    at.scale = kAttnScale;
    at.ldo = C;
    at.qkv = at.out = (void*)(uintptr_t)256;
    at.lse = (float*)(uintptr_t)256; at.bias_table = (const float*)(uintptr_t)256;
}
// The ONE place that picks the attention entry point of a block (GG_ATTN_ENTRY_*; the dtype code that goes with it is attn_dtype): the launches, the
// dbias_scratch sizing and the scratch.attn_ds plan all ask it, and gg_attention_route then says what that entry runs.  fp32 / fp32_split: the flash pair.
// bf16: gg_attention_fwd / _bwd -- except, under the opt-in switches, the windows gg_attention_fwd itself hands to the online-softmax forward (what its
// route reports: beyond 256 tokens), which take the 16-bit-MFMA window kernels: any forward under attn16 or attn16_train, the backward under attn16_train
// (a compacted block -- window_map -- is an fp32_split form and never meets the switch).
static int attn_entry(bool f32, bool attn16, bool attn16_train, const GgAttnArgs& at, bool bwd) {
    if (f32) return bwd ? GG_ATTN_ENTRY_FLASH_BWD : GG_ATTN_ENTRY_FLASH_FWD;
    GgAttnRoute fwd;
    if ((bwd ? attn16_train && !at.window_map : attn16 || attn16_train) && gg_attention_route(&at, GG_ATTN_ENTRY_FWD, 0, &fwd) == 0 &&
        (fwd.kernel == GG_ATTN_KERNEL_FLASH_FWD_STREAM || fwd.kernel == GG_ATTN_KERNEL_FLASH_FWD_RESIDENT))
        return bwd ? GG_ATTN_ENTRY_FLASH16_WIN_BWD : GG_ATTN_ENTRY_FLASH16_WIN_FWD;
    return bwd ? GG_ATTN_ENTRY_BWD : GG_ATTN_ENTRY_FWD;
}
static int attn_dtype(bool f32) { return f32 ? 1 : 0; }

// Which fused forms the schedule takes.  The workspace plan decides who owns the tensors a fusion removes and the executor decides who writes
// them, so there is ONE value per C-ABI call: build_model fills Model::sch from the storage type and the dev switches, both read it there.
struct Schedule { bool fuse_dw_s2, fuse_dw_s1, fuse_bnbwd, fuse_bnbwd_epi, fuse_bngemm, fuse_pro, fuse_lncol, fuse_lnbn; };
static Schedule schedule_flags(bool f32) {
    Schedule k;
    // the stride-2 depthwise conv of PatchMerging walks down the map with a 3x3 window per output column: BatchNorm1 + GELU are applied to
    // every loaded element (6 loads per step where 4 are new: 1.5 evaluations per input element), the apply pass and the activation tensor disappear
    k.fuse_dw_s2 = gg_dev_env("GG_NO_FUSE_DW_S2") == nullptr;
    // MBConv.conv2 likewise through the 4-columns-per-thread stride-1 kernel (1.5 BatchNorm+GELU evaluations per input element)
    k.fuse_dw_s1 = gg_dev_env("GG_NO_FUSE_DW_S1") == nullptr;
    // Frozen depthwise taps: the data gradient forms BatchNorm backward's apply step (dy = c0*dz + c1*y + c2) while it loads its
    // input, and (MBConv) emits dz = da*act'(BN(y)) + the reduce sums of the ConvNorm in front: apply and reduce passes and
    // the dy / da tensors disappear.  GG_NO_FUSE_BNBWD=1 / GG_NO_FUSE_BNBWD_EPI=1 restore the separate passes.
    k.fuse_bnbwd = gg_dev_env("GG_NO_FUSE_BNBWD") == nullptr;
    k.fuse_bnbwd_epi = gg_dev_env("GG_NO_FUSE_BNBWD_EPI") == nullptr;
    // Frozen ConvNorm chains: BatchNorm backward's reduce rides in the epilogue of the conv dgrad that produces its input
    // gradient, and its apply step is folded into the weights of the 1x1 dgrad that consumes its output gradient.
    k.fuse_bngemm = gg_dev_env("GG_NO_BNGEMM") == nullptr;
    k.fuse_pro = gg_dev_env("GG_NO_PRO") == nullptr;              // MBConv conv3 applies BatchNorm2 + GELU in its A prologue (one N tile: each element is transformed once)
    k.fuse_lncol = gg_dev_env("GG_NO_LN_COLSUM") == nullptr;      // norm2's backward leaves local_conv's BatchNorm-backward column sums (frozen blocks)
    k.fuse_lnbn = true;                                           // f32 storage: local_conv's BatchNorm apply inside norm2
    // f32 storage takes the same fusions where an f32 twin exists (MBConv / PatchMerging forward, the stride-1 data gradients, the GEMM-side
    // BatchNorm epilogue / prologues); GG_F32_NO_FUSE=1 runs every BatchNorm pass on its own (the schedule the fusions are tested against)
    if (f32 && gg_dev_env("GG_F32_NO_FUSE")) k = Schedule{};
    return k;
}
// One unit of the schedule (and of activation recompute): an MBConv of stage 0, the PatchMerging of stage 1..3, a TinyVitBlock of stage 1..3
enum { SEG_MBCONV, SEG_MERGE, SEG_BLOCK };
struct Segment { int kind, stage, index, slot; };       // slot: its first DropPath slot (an MBConv has one, a block two, a PatchMerging none)

struct Model {
    GgTinyVitCfg cfg;
    Schedule sch;
    std::vector<Segment> segs;      // in forward order; the backward walks it from the end
    int drop_slots = 0;
    int es = 2;             // bytes per activation / cached-weight element: 2 (bf16) or 4 (f32, reference-precision mode)
    bool f32 = false;
    bool split = false;     // act_dtype 3 ("fp32_split"): f32 storage and arithmetic; the Linears of the transformer blocks (forward and data gradients) run as fp32-accurate
                            // split products on the bf16 MFMA -- the activation operand split while the kernel stages it, the weight as cached planes
    struct PlaneOf { int64_t w, planes; int rows, ld; };      // cached f32 matrix at wcache offset w ([rows][ld]) -> its bf16 planes [3][rows][ld]
    std::vector<PlaneOf> plane_of;
    std::vector<TensorInfo> tensors;
    int64_t param_floats = 0, buffer_floats = 0, wcache_bytes = 0;
    int num_counters = 0;
    ConvBNDense pe1, pe2;
    std::vector<MBConvL> mb;
    StageL stages[3];
    LNP head;
    int res0;   // spatial size of stage 0 (img/4)
};

static int add_tensor(Model& m, const std::string& name, std::initializer_list<int64_t> shape, int kind) {
    TensorInfo t;
    t.name = name; t.kind = kind; t.ndim = (int)shape.size(); t.numel = 1;
    int i = 0;
    for (int j = 0; j < 4; ++j) t.shape[j] = 1;
    for (auto s : shape) { t.shape[i++] = s; t.numel *= s; }
    if (kind == GG_KIND_PARAM) { t.offset = m.param_floats; m.param_floats += gg_align(t.numel, 8); }
    else if (kind == GG_KIND_BUFFER) { t.offset = m.buffer_floats; m.buffer_floats += gg_align(t.numel, 8); }
    else { t.offset = m.num_counters++; }
    m.tensors.push_back(t);
    return (int)m.tensors.size() - 1;
}
static int64_t wc_alloc(Model& m, int64_t bytes) {
    int64_t o = m.wcache_bytes;
    m.wcache_bytes += gg_align(bytes, 256);
    return o;
}
static void make_dense(Model& m, DenseW& w, const std::string& wname, int N, int cin, int taps, const std::string* bname, bool conv) {
    w.N = N; w.cin = cin; w.taps = taps; w.K = cin * taps; w.Kp = (int)gg_align(w.K, 8); w.Np = (int)gg_align(N, 8);
    if (conv) { const int ks = taps == 9 ? 3 : 1; w.t_w = add_tensor(m, wname, {N, cin, ks, ks}, GG_KIND_PARAM); }
    else w.t_w = add_tensor(m, wname, {N, cin}, GG_KIND_PARAM);
    if (bname) w.t_b = add_tensor(m, *bname, {N}, GG_KIND_PARAM);
    w.wn = wc_alloc(m, (int64_t)N * w.Kp * m.es);
    w.wt = wc_alloc(m, (int64_t)w.Kp * w.Np * m.es);
}
static void make_bn(Model& m, BNP& bn, const std::string& prefix, int C) {
    bn.C = C;
    bn.t_g = add_tensor(m, prefix + ".bn.weight", {C}, GG_KIND_PARAM);
    bn.t_b = add_tensor(m, prefix + ".bn.bias", {C}, GG_KIND_PARAM);
    bn.rm = m.tensors[add_tensor(m, prefix + ".bn.running_mean", {C}, GG_KIND_BUFFER)].offset;
    bn.rv = m.tensors[add_tensor(m, prefix + ".bn.running_var", {C}, GG_KIND_BUFFER)].offset;
    bn.cnt = (int)m.tensors[add_tensor(m, prefix + ".bn.num_batches_tracked", {}, GG_KIND_COUNTER)].offset;
}
static void make_convbn_dense(Model& m, ConvBNDense& c, const std::string& prefix, int cin, int cout, int taps) {
    make_dense(m, c.w, prefix + ".conv.weight", cout, cin, taps, nullptr, true);
    make_bn(m, c.bn, prefix, cout);
    if (m.split) {      // planes of W: the forward of a ConvNorm's dense convolution (plain epilogue + BatchNorm partials) runs as a split product
        c.w.wn3 = wc_alloc(m, (int64_t)3 * c.w.N * c.w.Kp * 2);
        m.plane_of.push_back({c.w.wn, c.w.wn3, c.w.N, c.w.Kp});
        c.w.wt3 = wc_alloc(m, (int64_t)3 * c.w.Kp * c.w.Np * 2);      // ... and of W^T: the data gradients that go through the plain / Linear epilogues
        m.plane_of.push_back({c.w.wt, c.w.wt3, c.w.Kp, c.w.Np});
    }
}
static void make_convbn_dw(Model& m, ConvBNDw& c, const std::string& prefix, int C) {
    c.w.C = C;
    c.w.t_w = add_tensor(m, prefix + ".conv.weight", {C, 1, 3, 3}, GG_KIND_PARAM);
    c.w.taps = wc_alloc(m, (int64_t)9 * C * 4);
    make_bn(m, c.bn, prefix, C);
}
static void make_ln(Model& m, LNP& l, const std::string& prefix, int C) {
    l.C = C;
    l.t_g = add_tensor(m, prefix + ".weight", {C}, GG_KIND_PARAM);
    l.t_b = add_tensor(m, prefix + ".bias", {C}, GG_KIND_PARAM);
}

static int build_model(const GgTinyVitCfg* cfg, Model& m) {
    GG_CHECK(cfg, "tinyvit: null config");
    m.cfg = *cfg;
    GG_CHECK(cfg->act_dtype == 0 || cfg->act_dtype == 1 || cfg->act_dtype == 3, "tinyvit: act_dtype must be 0 (bf16), 1 (f32) or 3 (f32 storage, split-bf16 Linears)");
    m.f32 = cfg->act_dtype != 0; m.split = cfg->act_dtype == 3; m.es = m.f32 ? 4 : 2;
    m.sch = schedule_flags(m.f32);
    const int* d = cfg->embed_dims;
    GG_CHECK(cfg->img_size > 0 && cfg->img_size % 32 == 0, "tinyvit: img_size must be a multiple of 32");
    GG_CHECK(cfg->in_chans == 3, "tinyvit: in_chans must be 3");
    for (int s = 0; s < 4; ++s) {
        GG_CHECK(d[s] > 0 && d[s] % 16 == 0, "tinyvit: embed_dims[%d]=%d must be a multiple of 16", s, d[s]);
        GG_CHECK(cfg->depths[s] > 0, "tinyvit: depths[%d] must be > 0", s);
        if (s > 0) GG_CHECK(d[s] == cfg->num_heads[s] * 32, "tinyvit: head_dim must be 32 (dim %d, heads %d)", d[s], cfg->num_heads[s]);
    }
    m.res0 = cfg->img_size / 4;
    make_convbn_dense(m, m.pe1, "patch_embed.conv1", cfg->in_chans, d[0] / 2, 9);
    make_convbn_dense(m, m.pe2, "patch_embed.conv2", d[0] / 2, d[0], 9);
    const int mid = (int)(d[0] * cfg->mbconv_expand_ratio);
    GG_CHECK(mid % 8 == 0, "tinyvit: mbconv mid channels must be a multiple of 8");
    m.mb.resize(cfg->depths[0]);
    for (int i = 0; i < cfg->depths[0]; ++i) {
        const std::string p = "stages.0.blocks." + std::to_string(i);
        make_convbn_dense(m, m.mb[i].c1, p + ".conv1", d[0], mid, 1);
        make_convbn_dw(m, m.mb[i].c2, p + ".conv2", mid);
        make_convbn_dense(m, m.mb[i].c3, p + ".conv3", mid, d[0], 1);
        m.segs.push_back({SEG_MBCONV, 0, i, m.drop_slots});
        m.drop_slots += 1;
    }
    int res = m.res0;
    for (int s = 1; s < 4; ++s) {
        StageL& st = m.stages[s - 1];
        const int C = d[s], ws = cfg->window_sizes[s], nh = cfg->num_heads[s];
        res /= 2;
        GG_CHECK(ws > 0, "tinyvit: window_sizes[%d] must be > 0", s);
        st.C = C; st.heads = nh; st.ws = ws; st.res = res; st.pres = (int)gg_align(res, ws);
        GG_CHECK(ws <= 32, "tinyvit: window %d unsupported (max 32x32 tokens)", ws);
        const std::string pm = "stages." + std::to_string(s) + ".downsample";
        make_convbn_dense(m, st.merge.c1, pm + ".conv1", d[s - 1], C, 1);
        make_convbn_dw(m, st.merge.c2, pm + ".conv2", C);
        make_convbn_dense(m, st.merge.c3, pm + ".conv3", C, C, 1);
        m.segs.push_back({SEG_MERGE, s, 0, m.drop_slots});
        const int hid = (int)(C * cfg->mlp_ratio);
        st.blocks.resize(cfg->depths[s]);
        for (int i = 0; i < cfg->depths[s]; ++i) {
            BlockL& b = st.blocks[i];
            const std::string p = "stages." + std::to_string(s) + ".blocks." + std::to_string(i);
            b.t_ab = add_tensor(m, p + ".attn.attention_biases", {nh, ws * ws}, GG_KIND_PARAM);
            if (!m.f32 && ws <= 16) {     // expanded bf16 table of the register-resident kernels; the flash kernels read the compact parameter
                const int np_ = gg_attention_padded_tokens(ws * ws);
                b.bias_full = wc_alloc(m, (int64_t)nh * np_ * np_ * 2);
            } else b.bias_full = -1;
            make_ln(m, b.ln1, p + ".attn.norm", C);
            std::string bn = p + ".attn.qkv.bias";
            make_dense(m, b.qkv, p + ".attn.qkv.weight", 3 * C, C, 1, &bn, false);
            bn = p + ".attn.proj.bias";
            make_dense(m, b.proj, p + ".attn.proj.weight", C, C, 1, &bn, false);
            make_ln(m, b.ln2, p + ".mlp.norm", C);
            bn = p + ".mlp.fc1.bias";
            make_dense(m, b.fc1, p + ".mlp.fc1.weight", hid, C, 1, &bn, false);
            bn = p + ".mlp.fc2.bias";
            make_dense(m, b.fc2, p + ".mlp.fc2.weight", C, hid, 1, &bn, false);
            make_convbn_dw(m, b.local, p + ".local_conv", C);
            m.segs.push_back({SEG_BLOCK, s, i, m.drop_slots});
            m.drop_slots += 2;
            if (m.split) {      // bf16 planes of W and W^T of the block's four Linears (B operand of gg_gemm_nt_split3_af32: forward and data gradients)
                for (DenseW* w : {&b.qkv, &b.proj, &b.fc1, &b.fc2}) {
                    w->wn3 = wc_alloc(m, (int64_t)3 * w->N * w->Kp * 2);
                    w->wt3 = wc_alloc(m, (int64_t)3 * w->Kp * w->Np * 2);
                    m.plane_of.push_back({w->wn, w->wn3, w->N, w->Kp});
                    m.plane_of.push_back({w->wt, w->wt3, w->Kp, w->Np});
                }
            }
        }
    }
    make_ln(m, m.head, "head.norm", d[3]);
    return 0;
}

// ------------------------------------------------------------------------------------------- workspace plan
struct Region { std::string name; int64_t offset, bytes; };
struct Plan {
    bool training = true;
    bool dry = true;
    std::vector<Region> regs;
    std::map<std::string, int> index;
    int64_t total = 0;
    int64_t max_transient = 0;
    int ring_next = 0;
    int64_t ring_base = 0;
    static constexpr int RING = 10;
    // Training-time temporaries: tensors that live only between their producer and their one consumer because -- under the trainable mask the plan
    // was made for -- no weight gradient reads them (the input of a frozen Linear / depthwise conv, the activation tensors the fused forward never
    // writes).  They alternate between TRING slots of the largest one; `temps` holds their names (gg_tinyvit_activation_info refuses them).
    const uint8_t* mask = nullptr;       // one byte per tensor of the model, or null = everything trainable
    int64_t max_temp = 0, temp_base = 0, gbytes_seen = 0;
    int temp_next = 0;
    bool alias_G = false;
    static constexpr int TRING = 2;
    std::map<std::string, int> temps;
    bool tr(int t) const { return mask == nullptr || mask[t] != 0; }
    int64_t alloc_temp(const std::string& name, int64_t bytes) {
        if (!training) return alloc(name, bytes, true);
        bytes = gg_align(std::max<int64_t>(bytes, 16), 256);
        max_temp = std::max(max_temp, bytes);
        const int64_t off = dry ? 0 : temp_base + (int64_t)(temp_next % TRING) * max_temp;
        temp_next++;
        temps[name] = 1;
        index[name] = (int)regs.size();
        regs.push_back({name, off, bytes});
        return off;
    }
    // act1 behind a fused forward with trainable taps: never written in forward, re-formed by backward right before the tap gradient reads it -- all
    // such layers share ONE region (they are processed one at a time)
    int64_t max_shared = 0, shared_base = 0;
    int64_t alloc_shared(const std::string& name, int64_t bytes) {
        if (!training) return alloc(name, bytes, true);
        bytes = gg_align(std::max<int64_t>(bytes, 16), 256);
        max_shared = std::max(max_shared, bytes);
        temps[name] = 1;
        index[name] = (int)regs.size();
        regs.push_back({name, shared_base, bytes});
        return shared_base;
    }
    // Activation recompute (GgTinyVitCfg.recompute = 1, training): the tensors inside a segment (an MBConv, a PatchMerging, a TinyVitBlock) --
    // everything but its output and its ConvNorms' .stat -- are laid out from the start of ONE segment region that every segment reuses (the
    // backward re-forms a segment's tensors there right before its backward).  The frozen-mask temporaries and the re-formed act1 live there too:
    // no ring, no gradient buffer aliases them.  `recomputed` holds their names (gg_tinyvit_activation_info refuses them).
    bool rc = false;
    int ds_force = -1;                   // rc: whether scratch.attn_ds exists is taken from the recompute-off plan (1 / 0; -1: decided here)
    int64_t seg_base = 0, seg_cur = 0, max_seg = 0;
    std::map<std::string, int> recomputed;
    void seg_begin() { seg_cur = 0; }
    int64_t alloc_seg(const std::string& name, int64_t bytes) {
        bytes = gg_align(std::max<int64_t>(bytes, 16), 256);
        const int64_t off = dry ? 0 : seg_base + seg_cur;
        seg_cur += bytes;
        max_seg = std::max(max_seg, seg_cur);
        recomputed[name] = 1;
        index[name] = (int)regs.size();
        regs.push_back({name, off, bytes});
        return off;
    }
    // a segment-internal tensor: the segment region under recompute, else its own storage (training) / the inference ring
    int64_t alloc_in(const std::string& name, int64_t bytes) { return rc ? alloc_seg(name, bytes) : alloc(name, bytes); }
    // persistent: always gets its own storage; transient activations share a ring in inference mode
    int64_t alloc(const std::string& name, int64_t bytes, bool transient = true) {
        bytes = gg_align(std::max<int64_t>(bytes, 16), 256);
        int64_t off;
        if (!training && transient) {
            max_transient = std::max(max_transient, bytes);
            off = dry ? 0 : ring_base + (int64_t)(ring_next % RING) * max_transient;
            ring_next++;
        } else {
            off = total;
            total += bytes;
        }
        index[name] = (int)regs.size();
        regs.push_back({name, off, bytes});
        return off;
    }
};

struct Act {   // offsets (bytes) of the saved tensors of one ConvNorm
    int64_t y = 0, stat = 0;
};
struct MBAct { int64_t x, a1, a2, out; Act c1, c2, c3; };
struct MergeAct { int64_t a1, a2, out; Act c1, c2, c3; };
struct BlockAct { int64_t x0, a, mean1, rstd1, qkv, o, lse, x1, x2, b, mean2, rstd2, hpre, h, x3; Act local;
                  int64_t xpad = -1; };      // padded block (pres != res): x0 zero-padded to the padded map; a / mean1 / rstd1 / qkv / o / lse then hold B * pres^2 rows in padded map order
struct Layout {
    int64_t col1, col2, x_pe; Act pe1, pe2;
    std::vector<MBAct> mb;
    MergeAct merge[3];
    std::vector<BlockAct> blocks[3];
    int64_t pooled, mean_h, rstd_h;
    // scratch
    int64_t statpart, bnscratch, lnscratch, colsum, splitk, attn_ds = -1, G[5];
    int64_t padtmp = -1;         // padded blocks: proj's output on the padded map, between the GEMM and the crop (one region for all of them; absent when every map divides)
    int64_t foldw, foldb;        // BatchNorm-backward-folded dgrad weights bf16 [Cin][2*Cout] and bias f32 [Cin]
    int64_t colsum_bytes = 0;    // (scratch.colsum also holds the two kept lists of a compacted block while that block runs: block_compacts)
    int64_t gbytes;
};

static int64_t bn_part_floats(int64_t M, int C, int B, int Ho, int Wo, bool dw) {
    const int rows = dw ? std::max(std::max(gg_dwconv_stat_rows(B, Ho, Wo, C, 1), gg_dwconv_stat_rows(B, Ho, Wo, C, 2)),
                                   std::max(gg_dwconv_fused_stat_rows(B, Ho, Wo, C, 1), gg_dwconv_fwd_fused_stat_rows(B, Ho, Wo, C, 1)))
                        : gg_gemm_colstats_rows((int)M);
    return (int64_t)gg_stat_rows_capacity(rows) * 2 * C;
}

// The forward routes that decide who writes act1 / act2 of an MBConv or a PatchMerging: the plan gives those tensors their storage by the same
// predicates the forward (and the backward, where it re-forms act1 for the tap gradient) takes its route by.
// act1 = GELU(BN1(y1)) is never written by the forward: the depthwise conv (stride 1: MBConv, 2: PatchMerging) forms it while staging its input
static bool act1_fused_away(const Schedule& k, int stride) { return stride == 1 ? k.fuse_dw_s1 : k.fuse_dw_s2; }
// MBConv conv3 reads BN2 + GELU of conv2's output through its A prologue and act2 is not written -- unless conv3's weight gradient needs that
// tensor (w_trains: training and conv3.weight trainable; the plan keeps act2 then, and makes it a temporary otherwise whichever route is taken)
static bool conv3_takes_prologue(const Schedule& k, const DenseW& w, int mid, bool w_trains) {
    return k.fuse_pro && !w_trains && w.Kp == mid && mid <= 1024 && w.N <= 128;
}

static void plan_build(const Model& m, int B, Plan& p, Layout& L) {
    const GgTinyVitCfg& c = m.cfg;
    const int* d = c.embed_dims;
    const int H1 = c.img_size / 2, H0 = m.res0;
    const int64_t M1 = (int64_t)B * H1 * H1, M0 = (int64_t)B * H0 * H0;
    int64_t gmax = 0, statmax = 0, bnsmax = 0, lnsmax = 0, csmax = 0, padmax = 0;
    const int64_t es = m.es;
    auto track = [&](int64_t elems) { gmax = std::max(gmax, elems * es); };
    auto bnreg = [&](const std::string& n, Act& a, int64_t M, int C, bool dw, int Bn, int Ho, int Wo, bool seg = true) {
        a.y = seg ? p.alloc_in(n + ".y", M * C * es) : p.alloc(n + ".y", M * C * es);
        a.stat = p.alloc(n + ".stat", 2 * C * 4, false);
        statmax = std::max(statmax, bn_part_floats(M, C, Bn, Ho, Wo, dw) * 4);
        if (dw) statmax = std::max(statmax, (int64_t)gg_stat_rows_capacity(std::max(gg_dwconv_f32_stat_rows(Bn, Ho, Wo, C, 1), gg_dwconv_f32_stat_rows(Bn, Ho, Wo, C, 2))) * 2 * C * 4);
        statmax = std::max(statmax, (int64_t)gg_stat_rows_capacity(4096) * 2 * C * 4);      // stride-2 fused data gradient partials
        bnsmax = std::max(bnsmax, gg_bn_bwd_scratch_floats(M, C) * 4);
        track(M * C);
    };
    L.col1 = p.alloc("patch_embed.col1", M1 * 32 * es);
    bnreg("patch_embed.conv1", L.pe1, M1, d[0] / 2, false, B, H1, H1, false);      // (PatchEmbed is kept whole under recompute too)
    L.col2 = p.alloc("patch_embed.col2", M0 * m.pe2.w.Kp * es);
    track(M0 * m.pe2.w.Kp); track(M1 * 32);
    bnreg("patch_embed.conv2", L.pe2, M0, d[0], false, B, H0, H0, false);
    L.x_pe = p.alloc("patch_embed.out", M0 * d[0] * es);
    const int mid = (int)(d[0] * c.mbconv_expand_ratio);
    L.mb.resize(m.mb.size());
    int64_t prev = L.x_pe;
    for (size_t i = 0; i < m.mb.size(); ++i) {
        const std::string n = "stages.0.blocks." + std::to_string(i);
        MBAct& a = L.mb[i];
        a.x = prev;
        // act1 = GELU(BN1(y1)): the fused depthwise forward never writes it (backward re-forms it as a temporary when conv2's taps train); unfused, it
        // is read again only by conv2's weight gradient.  act2 = GELU(BN2(y2)): conv3's input, kept only for conv3's weight gradient.
        const MBConvL& ml = m.mb[i];
        p.seg_begin();
        bnreg(n + ".conv1", a.c1, M0, mid, false, B, H0, H0);
        a.a1 = p.rc ? p.alloc_seg(n + ".act1", M0 * mid * es) : !p.tr(ml.c2.w.t_w) ? p.alloc_temp(n + ".act1", M0 * mid * es) : act1_fused_away(m.sch, 1) ? p.alloc_shared(n + ".act1", M0 * mid * es) : p.alloc(n + ".act1", M0 * mid * es);
        bnreg(n + ".conv2", a.c2, M0, mid, true, B, H0, H0);
        a.a2 = p.rc ? p.alloc_seg(n + ".act2", M0 * mid * es) : !p.tr(ml.c3.w.t_w) ? p.alloc_temp(n + ".act2", M0 * mid * es) : p.alloc(n + ".act2", M0 * mid * es);
        bnreg(n + ".conv3", a.c3, M0, d[0], false, B, H0, H0);
        a.out = p.alloc(n + ".out", M0 * d[0] * es);
        prev = a.out;
    }
    int res = H0;
    int64_t Mprev = M0;
    for (int s = 0; s < 3; ++s) {
        const StageL& st = m.stages[s];
        const int C = st.C;
        const int64_t M = (int64_t)B * st.res * st.res, Mp = (int64_t)B * st.pres * st.pres;      // Mp: rows of the attention branch (= M unless the map is padded)
        const std::string n = "stages." + std::to_string(s + 1) + ".downsample";
        MergeAct& ma = L.merge[s];
        p.seg_begin();
        bnreg(n + ".conv1", ma.c1, Mprev, C, false, B, res, res);
        ma.a1 = p.rc ? p.alloc_seg(n + ".act1", Mprev * C * es) : !p.tr(st.merge.c2.w.t_w) ? p.alloc_temp(n + ".act1", Mprev * C * es) : act1_fused_away(m.sch, 2) ? p.alloc_shared(n + ".act1", Mprev * C * es) : p.alloc(n + ".act1", Mprev * C * es);
        bnreg(n + ".conv2", ma.c2, M, C, true, B, st.res, st.res);
        ma.a2 = p.rc ? p.alloc_seg(n + ".act2", M * C * es) : !p.tr(st.merge.c3.w.t_w) ? p.alloc_temp(n + ".act2", M * C * es) : p.alloc(n + ".act2", M * C * es);
        bnreg(n + ".conv3", ma.c3, M, C, false, B, st.res, st.res);
        ma.out = p.alloc(n + ".out", M * C * es);
        prev = ma.out;
        const int hid = (int)(C * c.mlp_ratio);
        L.blocks[s].resize(st.blocks.size());
        for (size_t i = 0; i < st.blocks.size(); ++i) {
            const std::string bn = "stages." + std::to_string(s + 1) + ".blocks." + std::to_string(i);
            BlockAct& a = L.blocks[s][i];
            const BlockL& bl = st.blocks[i];
            a.x0 = prev;
            // inputs of frozen Linears / of the frozen local conv are consumed once, right after they are written: ln1 -> qkv, x1 -> local_conv,
            // ln2 -> fc1, GELU(fc1) -> fc2 (the backward of a frozen block needs x0 / x2 / means for the LayerNorms, qkv / o / lse for the attention,
            // local_conv.y for its BatchNorm and the fc1 pre-activation for GELU'): 7 C of the block's 19 C floats per token
            p.seg_begin();
            auto keep = [&](bool trains, const std::string& nm, int64_t bytes) { return p.rc ? p.alloc_seg(nm, bytes) : !trains ? p.alloc_temp(nm, bytes) : p.alloc(nm, bytes); };
            // padded block: the attention branch runs on the zero-padded map (Mp rows).  xpad is LayerNorm1's input: the backward reads it again, and re-forms it from x0
            // when neither LayerNorm1 nor qkv trains (then it is a temporary like ln1)
            if (st.pres != st.res) {
                a.xpad = keep(p.tr(bl.qkv.t_w) || p.tr(bl.ln1.t_g), bn + ".attn.xpad", Mp * C * es);
                padmax = std::max(padmax, Mp * C * es);
                track(Mp * 3 * C);
            }
            a.a = keep(p.tr(bl.qkv.t_w), bn + ".ln1", Mp * C * es);
            a.mean1 = p.alloc_in(bn + ".mean1", Mp * 4);
            a.rstd1 = p.alloc_in(bn + ".rstd1", Mp * 4);
            a.qkv = p.alloc_in(bn + ".qkv", Mp * 3 * C * es);
            a.o = p.alloc_in(bn + ".attn.out", Mp * C * es);
            a.lse = p.alloc_in(bn + ".attn.lse", Mp * st.heads * 4);
            a.x1 = keep(p.tr(bl.local.w.t_w), bn + ".x1", M * C * es);
            bnreg(bn + ".local_conv", a.local, M, C, true, B, st.res, st.res);
            a.x2 = p.alloc_in(bn + ".x2", M * C * es);
            a.b = keep(p.tr(bl.fc1.t_w), bn + ".ln2", M * C * es);
            a.mean2 = p.alloc_in(bn + ".mean2", M * 4);
            a.rstd2 = p.alloc_in(bn + ".rstd2", M * 4);
            a.hpre = p.alloc_in(bn + ".fc1.pre", M * hid * es);
            a.h = keep(p.tr(bl.fc2.t_w), bn + ".fc1.act", M * hid * es);
            a.x3 = p.alloc(bn + ".out", M * C * es);
            prev = a.x3;
            track(M * hid); track(M * 3 * C);
            lnsmax = std::max(lnsmax, gg_layernorm_bwd_scratch_floats(Mp, C) * 4);
            csmax = std::max(csmax, gg_colsum_scratch_floats((int)M, hid) * 4);
            csmax = std::max(csmax, gg_colsum_scratch_floats((int)Mp, 3 * C) * 4);
        }
        res = st.res;
        Mprev = M;
    }
    L.pooled = p.alloc("head.pooled", (int64_t)B * d[3] * 4, false);
    L.mean_h = p.alloc("head.mean", (int64_t)B * 4, false);
    L.rstd_h = p.alloc("head.rstd", (int64_t)B * 4, false);
    lnsmax = std::max(lnsmax, gg_layernorm_bwd_scratch_floats(B, d[3]) * 4);
    L.statpart = p.alloc("scratch.statpart", statmax, false);
    if (padmax > 0) L.padtmp = p.alloc("scratch.padtmp", padmax, false);
    if (p.training) {
        // dw wgrad scratch may exceed the BN scratch
        int64_t dwmax = 0;
        dwmax = std::max(dwmax, gg_dwconv_wgrad_scratch_floats(B, H0, H0, mid, 1) * 4);
        dwmax = std::max(dwmax, gg_dwconv_f32_wgrad_scratch_floats(B, H0, H0, mid, 1) * 4);
        for (int s = 0; s < 3; ++s) {
            const int rin = s == 0 ? H0 : m.stages[s - 1].res;
            dwmax = std::max(dwmax, gg_dwconv_wgrad_scratch_floats(B, rin, rin, m.stages[s].C, 2) * 4);
            dwmax = std::max(dwmax, gg_dwconv_wgrad_scratch_floats(B, m.stages[s].res, m.stages[s].res, m.stages[s].C, 1) * 4);
            dwmax = std::max(dwmax, gg_dwconv_f32_wgrad_scratch_floats(B, rin, rin, m.stages[s].C, 2) * 4);
            dwmax = std::max(dwmax, gg_dwconv_f32_wgrad_scratch_floats(B, m.stages[s].res, m.stages[s].res, m.stages[s].C, 1) * 4);
        }
        L.bnscratch = p.alloc("scratch.bn", std::max(bnsmax, dwmax), false);
        L.lnscratch = p.alloc("scratch.ln", lnsmax, false);
        L.colsum_bytes = std::max<int64_t>(csmax, 1024);
        L.colsum = p.alloc("scratch.colsum", L.colsum_bytes, false);
        L.splitk = p.alloc("scratch.splitk", (int64_t)128 << 20, false);      // gg_gemm_tn_f32_splits sizes its slabs against this
        if (m.f32) {     // dS hand-off between the two passes of the flash attention backward (GgAttnArgs.ds_scratch): the largest stage decides
            // only windows beyond 256 tokens use it (the single-pass backward keeps dS on the CU), and only while it stays a small part of the workspace:
            // at most 4 GB and 1/8 of what is planned so far (24 x 24 windows: 16 MB per image; 32 x 32: 50 MB per image -- there both passes recompute)
            int64_t dsmax = 0;
            for (int s = 1; s < 4; ++s) {
                const auto& st = m.stages[s - 1];
                const int nw = B * (st.pres / st.ws) * (st.pres / st.ws);
                // the route of this stage's backward with every optional tensor given (bias gradient included: the call with the largest LDS need, so the
                // one that leaves the single-pass kernels first -- DESIGN.md 5, "One attention route"): does it read a dS region?
                GgAttnArgs at;
                GgAttnRoute r;
                attn_shape(st, B, at);
                at.dout = at.qkv; at.lddo = at.ldo; at.dqkv = at.out; at.dbias = at.lse; at.ds_scratch = at.lse;
                if (gg_attention_route(&at, attn_entry(true, false, false, at, true), attn_dtype(true), &r) == 0 && r.reads_ds_scratch)
                    dsmax = std::max(dsmax, gg_attention_flash_ds_scratch_floats(nw, st.heads, st.ws * st.ws) * 4);
            }
            // (under recompute the recompute-off plan decides: p.total differs, and the region selects the flash backward's route)
            const bool ds = p.ds_force >= 0 ? p.ds_force == 1 : (dsmax > 0 && dsmax <= ((int64_t)4 << 30) && dsmax <= p.total / 8);
            if (ds) L.attn_ds = p.alloc("scratch.attn_ds", dsmax, false);
        }
        int64_t fold = (int64_t)d[0] * 2 * mid;
        for (int s = 0; s < 3; ++s) fold = std::max(fold, (int64_t)(s == 0 ? d[0] : m.stages[s - 1].C) * 2 * m.stages[s].C);
        L.foldw = p.alloc("scratch.foldw", fold * es, false);
        L.foldb = p.alloc("scratch.foldb", 4096 * 4, false);
        L.gbytes = gg_align(gmax, 256);
        p.gbytes_seen = L.gbytes;
        // the forward's temporaries are dead when backward starts and the first two gradient ping-pong buffers are untouched until then: they share
        // the ring's slots -- unless backward itself re-forms a temporary (act1 for a trainable depthwise conv behind a fused forward)
        for (int i = 0; i < 5; ++i) {
            if (i < Plan::TRING && p.alias_G && !p.dry) {
                L.G[i] = p.temp_base + (int64_t)i * p.max_temp;
                p.index["scratch.G" + std::to_string(i)] = (int)p.regs.size();
                p.regs.push_back({"scratch.G" + std::to_string(i), L.G[i], L.gbytes});
            } else L.G[i] = p.alloc("scratch.G" + std::to_string(i), L.gbytes, false);
        }
    }
}
static void plan_make(const Model& m, int B, bool training, Plan& p, Layout& L, const uint8_t* mask = nullptr, bool allow_rc = true) {
    if (training && allow_rc && m.cfg.recompute) {
        Plan off; Layout Loff;                     // the recompute-off plan: what it decides from its own size, the checkpointed one inherits
        plan_make(m, B, true, off, Loff, mask, false);
        Plan q;
        q.training = true; q.mask = mask; q.rc = true; q.ds_force = Loff.attn_ds >= 0 ? 1 : 0;
        Plan dry = q; Layout Ld;                   // first pass: the segment region's size; second pass: the region first, then the rest
        plan_build(m, B, dry, Ld);
        q.dry = false; q.seg_base = 0; q.total = dry.max_seg;
        plan_build(m, B, q, L);
        q.index["scratch.segment"] = (int)q.regs.size();
        q.regs.push_back({"scratch.segment", q.seg_base, q.max_seg});
        p = q;
        return;
    }
    p.training = training;
    p.dry = true;
    p.mask = training ? mask : nullptr;
    plan_build(m, B, p, L);
    if (training && (p.max_temp > 0 || p.max_shared > 0)) {
        Plan q;                                    // second pass: the temporaries' ring (= the first two gradient buffers) first, then the shared act1 region, then the rest
        q.training = true; q.dry = false; q.mask = p.mask; q.temp_base = 0;
        q.alias_G = p.max_temp > 0;
        q.max_temp = q.alias_G ? std::max(p.max_temp, p.gbytes_seen) : 0;
        q.shared_base = (int64_t)Plan::TRING * q.max_temp;
        q.total = q.shared_base + p.max_shared;
        Layout L2;
        plan_build(m, B, q, L2);
        p = q; L = L2;
    }
    if (!training) {
        Plan q;
        q.training = false; q.dry = false; q.max_transient = p.max_transient;
        q.ring_base = p.total;                     // persistent regions first, ring after
        Layout L2;
        plan_build(m, B, q, L2);
        q.total = q.ring_base + (int64_t)Plan::RING * q.max_transient;
        p = q; L = L2;
    }
}

// ------------------------------------------------------------------------------------------- execution context
typedef char act_t;        // an activation / cached-weight element of the model's storage type (bf16 or f32): only ever passed on
struct Exec {
    const Model* m; const Layout* L;
    int B; bool training;
    const float* params; float* buffers; int64_t* counters;
    const char* wc; char* ws; hipStream_t st;
    const float* drop;   // [slots][B] or null
    float* grads; const uint8_t* trainable;
    GgStageDoneFn stage_done = nullptr; void* stage_user = nullptr;     // host callback: the gradient of a stage is fully enqueued
    // activation recompute: the backward runs a segment's forward body again (mbconv_fwd / merge_fwd / block_fwd) -- no BatchNorm statistics are
    // finalised (the forward's .stat checkpoints are reused, the running buffers are not touched) and the segment's output is not rewritten
    bool replay = false;
    bool compact = false;   // DropPath row compaction is on for this call (the process-global switch, read once per call)
    bool det_dbias = false;         // backward, switch on (gg_tinyvit_set_deterministic_dbias): trainable attention_biases take gg_attention_dbias, the attention backward gets dbias = NULL
    bool attn16_train = false;      // training forward / backward, bf16, switch on (gg_tinyvit_set_attention16_train): the same windows through gg_attention_flash16_win_fwd / _bwd
    bool attn16 = false;    // gg_tinyvit_forward, inference, bf16, switch on (gg_tinyvit_set_attention16): windows beyond 256 tokens through gg_attention_flash16_win_fwd
    void done(int stage) const { if (stage_done) stage_done(stage, stage_user); }
    bool f32;               // reference-precision mode: f32 activations / cached weights, f32 MFMA
    Exec(const Model& model, const Layout& layout, int batch, bool train) : m(&model), L(&layout), B(batch), training(train), f32(model.f32) {}
    const Schedule& sch() const { return m->sch; }
    const float* P(int t) const { return params + m->tensors[t].offset; }
    float* Gd(int t) const { return grads + m->tensors[t].offset; }
    bool tr(int t) const { return trainable == nullptr || trainable[t] != 0; }
    act_t* A(int64_t off) const { return reinterpret_cast<act_t*>(ws + off); }
    float* F(int64_t off) const { return reinterpret_cast<float*>(ws + off); }
    const act_t* Wn(const DenseW& w) const { return reinterpret_cast<const act_t*>(wc + w.wn); }
    const act_t* Wt(const DenseW& w) const { return reinterpret_cast<const act_t*>(wc + w.wt); }
    const float* Taps(const DwW& w) const { return reinterpret_cast<const float*>(wc + w.taps); }
    const float* dropv(int slot) const { return drop ? drop + (int64_t)slot * B : nullptr; }
    // the kept lists of the block that is running (k = 0: its attention slot, 1: its MLP slot): [count, ...][kept][pos] (include/gg_drop.h).  They live in
    // scratch.colsum, which only the bias gradients of TRAINABLE Linears use: a compacted block is frozen, so nothing touches the region while it runs
    int* drop_list(int k) const { return reinterpret_cast<int*>(ws + L->colsum) + (int64_t)k * gg_drop_list_ints(B); }
};
// Row compaction of one Linear launch: the slot's kept list and which side(s) go through the row map (GgSplit3Args.groups_dev / a_map / c_map)
struct RowMap { const int* list; int rps; bool a, c; };

// 1x1-conv dgrad straight from (dz, y): BatchNorm backward's apply step is folded into the weights (gg_bn_bwd_fold_weights)
static int gemm_folded_dgrad(const Exec& e, const DenseW& w, const act_t* dz, const act_t* y, const float* coef, const float* stat,
                             act_t* dx, int64_t M, const act_t* residual) {
    const int Cout = w.N, Cin = w.K;
    if (e.f32) {
        // f32: a doubled contraction would cost real MFMA time (1/16 of the bf16 rate); instead the apply step dy = c0*dz + c1*y + c2 is formed
        // from the two sources while the register-staged GEMM stages its A tile (GgGemmArgs.A2 + a_bn_stat = coef)
        GgGemmArgs g;
        memset(&g, 0, sizeof(g));
        g.A = dz; g.lda = Cout; g.A2 = y; g.a_bn_stat = coef; g.B = e.Wt(w); g.ldb = w.Np; g.C = dx; g.ldc = Cin;
        g.M = (int)M; g.N = Cin; g.K = Cout; g.residual = residual; g.ldr = Cin;
        return gg_gemm_nt_f32(&g, e.st);
    }
    GG_TRY(gg_bn_bwd_fold_weights(e.P(w.t_w), coef, stat, Cout, Cin, e.A(e.L->foldw), e.F(e.L->foldb), e.st));
    GgGemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = dz; g.lda = Cout; g.A2 = y; g.k_split = Cout; g.B = e.A(e.L->foldw); g.ldb = 2 * Cout; g.C = dx; g.ldc = Cin;
    g.M = (int)M; g.N = Cin; g.K = 2 * Cout; g.bias = e.F(e.L->foldb); g.residual = residual; g.ldr = Cin;
    return gg_gemm_nt(&g, e.st);
}
// fp32_split mode: the split kernels need at least this many output tiles -- half the CUs' worth -- to beat the f32 GEMM, whose 64 x 64 tiles and
// split-K fill the chip where a 256- / 128-row split tile would leave most CUs idle
// (dev: GG_SPLIT_MIN_TILES lowers the threshold so that the oracle gate can take every split route at a batch the CPU oracle finishes in seconds)
static int64_t split_min_tiles() {
    static const char* env = gg_dev_env("GG_SPLIT_MIN_TILES");
    static const int64_t min_tiles = env ? atoll(env) : 128;
    return min_tiles;
}
// the cached bf16 planes of the f32 matrix W of the weight cache, if it has some that cover n rows at pitch ld; else null
static const Model::PlaneOf* planes_of(const Exec& e, const act_t* W, int64_t ld, int n) {
    const int64_t off = reinterpret_cast<const char*>(W) - e.wc;
    for (const Model::PlaneOf& po : e.m->plane_of)
        if (po.w == off) return po.ld == ld && po.rows >= n ? &po : nullptr;
    return nullptr;
}
static int gemm(const Exec& e, const act_t* A, int64_t lda, const act_t* Bm, int64_t ldb, void* C, int64_t ldc, int64_t M, int N, int K,
                const float* bias = nullptr, int act = 0, void* preact = nullptr, const float* rowscale = nullptr, int rps = 0,
                const act_t* residual = nullptr, float* colstats = nullptr, const act_t* dact_pre = nullptr, int dact = 0, const RowMap* rm = nullptr) {
    const int64_t split_tiles = ((M + (K >= 384 ? 255 : 127)) / (K >= 384 ? 256 : 128)) * ((N + 127) / 128);
    const Model::PlaneOf* po = nullptr;
    if (e.m->split && split_tiles >= split_min_tiles() && (K & 7) == 0 && (lda & 3) == 0 && (!colstats || !(bias || act || preact || rowscale || residual || dact_pre)))
        po = planes_of(e, Bm, ldb, N);
    if (po) {
        // fp32_split mode: a Linear whose weight operand has cached planes runs as a split product (A = the f32 activation itself, split in the kernel's loader)
        GgSplit3Args g;
        memset(&g, 0, sizeof(g));
        g.b_planes = e.wc + po->planes; g.ldb = ldb; g.M = (int)M; g.N = N; g.K = K; g.C = (float*)C; g.ldc = ldc;
        g.bias = bias; g.act = act; g.preact = (float*)preact; g.rowscale = rowscale; g.rows_per_scale = rps; g.residual = (const float*)residual; g.ldr = ldc;
        g.dact_preact = (const float*)dact_pre; g.dact = dact;
        if (rm) {
            g.groups_dev = rm->list; g.group_rows = rm->rps;
            g.a_map = rm->a ? rm->list + GG_DROP_LIST_HEAD : nullptr; g.c_map = rm->c ? rm->list + GG_DROP_LIST_HEAD : nullptr;
        }
        return gg_gemm_nt_split3_af32_stats(&g, (const float*)A, lda, (int64_t)po->rows * po->ld, colstats, e.st);
    }
    GG_CHECK(!rm, "tinyvit: a compacted Linear (M %lld N %d K %d) did not take the split route", (long long)M, N, K);
    GgGemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = A; g.lda = lda; g.B = Bm; g.ldb = ldb; g.C = C; g.ldc = ldc; g.M = (int)M; g.N = N; g.K = K;
    g.bias = bias; g.act = act; g.preact = preact; g.rowscale = rowscale; g.rows_per_scale = rps;
    g.residual = residual; g.ldr = ldc; g.colstats = colstats; g.dact_preact = dact_pre; g.dact = dact;
    return e.f32 ? gg_gemm_nt_f32(&g, e.st) : gg_gemm_nt(&g, e.st);
}

// BatchNorm statistics for a ConvNorm whose producer wrote `nparts` partial rows into statpart
static int bn_stats(const Exec& e, const BNP& bn, const Act& a, int nparts, int64_t count) {
    if (e.replay) return 0;      // recompute: (mean, rstd) are the forward's, already in a.stat
    if (e.training) {
        GG_TRY(gg_bn_finalize(e.F(e.L->statpart), nparts, bn.C, count, e.m->cfg.bn_eps, e.m->cfg.bn_momentum, e.F(a.stat),
                              e.buffers + bn.rm, e.buffers + bn.rv, e.st));
    } else {
        GG_TRY(gg_bn_eval_stat(e.buffers + bn.rm, e.buffers + bn.rv, bn.C, e.m->cfg.bn_eps, e.F(a.stat), e.st));
    }
    return 0;
}
// dense ConvNorm: y = A . Wn^T (+ partial stats) ; stat
static int conv_dense_fwd(const Exec& e, const ConvBNDense& c, const Act& a, const act_t* A, int64_t lda, int64_t M) {
    float* part = e.training ? e.F(e.L->statpart) : nullptr;
    GG_TRY(gemm(e, A, lda, e.Wn(c.w), c.w.Kp, e.A(a.y), c.w.N, M, c.w.N, c.w.Kp, nullptr, 0, nullptr, nullptr, 0, nullptr, part));
    return bn_stats(e, c.bn, a, gg_gemm_colstats_rows((int)M), M);
}
// dense ConvNorm whose input is act(BN(prev.y)) of the preceding ConvNorm, formed while the GEMM stages its A tile
static int conv_dense_fwd_pro(const Exec& e, const ConvBNDense& c, const Act& a, const BNP& prev_bn, const Act& prev, int in_act, int64_t M) {
    // fp32_split mode: the same fusion on the split kernels (the transform rides on the loader, in front of the split; 256-row tiles: K >= 384)
    static const char* nopro_env = gg_dev_env("GG_SPLIT3_NO_PRO");          // dev: the f32-MFMA prologue GEMM in the split mode too
    const Model::PlaneOf* po = nullptr;
    if (e.m->split && !nopro_env && c.w.Kp >= 384 && c.w.Kp <= 1024 && (c.w.Kp & 7) == 0 && ((M + 255) / 256) * ((c.w.N + 127) / 128) >= split_min_tiles())
        po = planes_of(e, e.Wn(c.w), c.w.Kp, c.w.N);
    if (po) {
        GgSplit3Args g;
        memset(&g, 0, sizeof(g));
        g.b_planes = e.wc + po->planes; g.ldb = c.w.Kp; g.M = (int)M; g.N = c.w.N; g.K = c.w.Kp; g.C = (float*)e.A(a.y); g.ldc = c.w.N;
        GG_TRY(gg_gemm_nt_split3_af32_pro(&g, (const float*)e.A(prev.y), c.w.Kp, (int64_t)po->rows * po->ld, e.F(prev.stat), e.P(prev_bn.t_g), e.P(prev_bn.t_b), in_act,
                                          e.training ? e.F(e.L->statpart) : nullptr, e.st));
        return bn_stats(e, c.bn, a, gg_gemm_colstats_rows((int)M), M);
    }
    GgGemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = e.A(prev.y); g.lda = c.w.Kp; g.B = e.Wn(c.w); g.ldb = c.w.Kp; g.C = e.A(a.y); g.ldc = c.w.N;
    g.M = (int)M; g.N = c.w.N; g.K = c.w.Kp;
    g.colstats = e.training ? e.F(e.L->statpart) : nullptr;
    g.a_bn_stat = e.F(prev.stat); g.a_bn_gamma = e.P(prev_bn.t_g); g.a_bn_beta = e.P(prev_bn.t_b); g.a_bn_act = in_act;
    GG_TRY(e.f32 ? gg_gemm_nt_f32(&g, e.st) : gg_gemm_nt(&g, e.st));
    return bn_stats(e, c.bn, a, gg_gemm_colstats_rows((int)M), M);
}
static int conv_dw_fwd(const Exec& e, const ConvBNDw& c, const Act& a, const act_t* x, int B, int H, int W, int stride) {
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    float* part = e.training ? e.F(e.L->statpart) : nullptr;
    if (e.f32) {
        GG_TRY(gg_dwconv3x3_fwd_f32((const float*)x, e.Taps(c.w), (float*)e.A(a.y), B, H, W, c.w.C, stride, part, e.st));
        return bn_stats(e, c.bn, a, gg_dwconv_f32_stat_rows(B, Ho, Wo, c.w.C, stride), (int64_t)B * Ho * Wo);
    }
    GG_TRY(gg_dwconv3x3_fwd(x, e.Taps(c.w), e.A(a.y), B, H, W, c.w.C, stride, part, e.st));
    return bn_stats(e, c.bn, a, gg_dwconv_stat_rows(B, Ho, Wo, c.w.C, stride), (int64_t)B * Ho * Wo);
}
// depthwise ConvNorm whose input is act(BN(prev.y)) of the preceding ConvNorm, formed on the fly while staging
static int conv_dw_fwd_fused(const Exec& e, const ConvBNDw& c, const Act& a, const BNP& prev_bn, const Act& prev, int in_act, int B, int H,
                             int W, int stride) {
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    float* part = e.training ? e.F(e.L->statpart) : nullptr;
    if (e.f32) {
        GG_TRY(gg_dwconv3x3_fwd_fused_f32((const float*)e.A(prev.y), e.F(prev.stat), e.P(prev_bn.t_g), e.P(prev_bn.t_b), in_act, e.Taps(c.w),
                                          (float*)e.A(a.y), B, H, W, c.w.C, stride, part, e.st));
        return bn_stats(e, c.bn, a, gg_dwconv_f32_stat_rows(B, Ho, Wo, c.w.C, stride), (int64_t)B * Ho * Wo);
    }
    GG_TRY(gg_dwconv3x3_fwd_fused(e.A(prev.y), e.F(prev.stat), e.P(prev_bn.t_g), e.P(prev_bn.t_b), in_act, e.Taps(c.w), e.A(a.y), B, H, W,
                                  c.w.C, stride, part, e.st));
    return bn_stats(e, c.bn, a, gg_dwconv_fwd_fused_stat_rows(B, H, W, c.w.C, stride), (int64_t)B * Ho * Wo);
}
static int bn_apply(const Exec& e, const BNP& bn, const Act& a, int64_t M, int act, act_t* out, const act_t* residual = nullptr,
                    const float* rowscale = nullptr, int rps = 0) {
    if (e.f32) return gg_bn_apply_f32((const float*)e.A(a.y), e.F(a.stat), e.P(bn.t_g), e.P(bn.t_b), M, bn.C, act, (const float*)residual,
                                      rowscale, rps, (float*)out, e.st);
    return gg_bn_apply(e.A(a.y), e.F(a.stat), e.P(bn.t_g), e.P(bn.t_b), M, bn.C, act, residual, rowscale, rps, out, e.st);
}
// window attention arguments of one TinyVitBlock (forward fields; the caller adds the backward ones)
static void attn_args(const Exec& e, const StageL& st, const BlockL& l, const BlockAct& a, int B, GgAttnArgs& at) {
    attn_shape(st, B, at);
    at.qkv = e.A(a.qkv);
    at.bias = l.bias_full >= 0 ? e.wc + l.bias_full : nullptr;      // expanded bf16 table (register-resident kernels)
    at.bias_table = e.P(l.t_ab);                                     // compact f32 parameter (online-softmax kernels)
    at.out = e.A(a.o); at.lse = e.F(a.lse);
}
static int attention_run(const Exec& e, const GgAttnArgs& at, bool bwd) {
    switch (attn_entry(e.f32, e.attn16, e.attn16_train, at, bwd)) {
        case GG_ATTN_ENTRY_FLASH_FWD: return gg_attention_flash_fwd(&at, attn_dtype(e.f32), e.st);
        case GG_ATTN_ENTRY_FLASH_BWD: return gg_attention_flash_bwd(&at, attn_dtype(e.f32), e.st);
        case GG_ATTN_ENTRY_FLASH16_WIN_FWD: return gg_attention_flash16_win_fwd(&at, 0, e.st);
        case GG_ATTN_ENTRY_FLASH16_WIN_BWD: return gg_attention_flash16_win_bwd(&at, 0, e.st);
        case GG_ATTN_ENTRY_BWD: return gg_attention_bwd(&at, e.st);
        default: return gg_attention_fwd(&at, e.st);
    }
}
static int attention_fwd(const Exec& e, const GgAttnArgs& at) { return attention_run(e, at, false); }
// The backward with its scratch: the bias gradient's partial rows go to the split-K region where the rows the route's second stage needs (at.dbias is set:
// the report is about this very call) fit 64 MB -- per-workgroup partials, a deterministic second stage; else float atomics -- and the planned dS region
// is passed along in the f32 modes (the route says whether it is read).
static int attention_bwd(const Exec& e, const StageL& st, GgAttnArgs& at) {
    const Layout& L = *e.L;
    GgAttnRoute r;
    if (at.dbias && e.det_dbias) {
        // the fixed-order bias gradient: dq / dk / dv from the route's backward without dbias (their bits do not depend on it), then the bias gradient alone
        // from the same qkv / out / lse / dout, with P as that route recomputes it; its partial rows take the split-K region
        GgAttnArgs db = at;
        const int64_t rows = gg_attention_dbias_rows(&db, attn_dtype(e.f32));
        if (rows < 0) return -1;
        const int64_t table_bytes = (int64_t)st.heads * st.ws * st.ws * 4, region = (int64_t)128 << 20;
        GG_CHECK(rows * table_bytes <= region / 2, "gg_tinyvit_backward: the fixed-order bias gradient's %lld partial rows do not fit the split-K region", (long long)rows);
        db.dbias_scratch = e.F(L.splitk);
        if (e.f32 && L.attn_ds >= 0 && !attn_switches().no_ds_scratch) at.ds_scratch = e.F(L.attn_ds);
        const int entry = attn_entry(e.f32, e.attn16, e.attn16_train, at, true);
        GG_TRY(gg_attention_route(&at, entry, attn_dtype(e.f32), &r));
        if (e.f32 && r.kernel == GG_ATTN_KERNEL_FLASH_BWD_SPLIT) {
            // the one exception: the f32 split single-pass kernel's two instantiations round dS's split residuals differently (dq / dk / dv differ by an ulp,
            // measured), so this route keeps the instantiation the switch-off step runs and lets it bin into a table nobody reads -- the last table-sized
            // piece of the region, with its partial rows in front where they fit the region's first half (else float atomics into that table)
            at.dbias = (float*)((char*)e.F(L.splitk) + region - gg_align(table_bytes, 256));
            if (r.dbias_rows * table_bytes <= region / 2) at.dbias_scratch = e.F(L.splitk);
        } else {
            at.dbias = nullptr;
            GG_TRY(gg_attention_route(&at, entry, attn_dtype(e.f32), &r));
        }
        GG_TRY(attention_run(e, at, true));
        // P must meet the forward's lse: the resident bf16 kernels start their scores from the expanded table, which holds bf16(bias / scale), like the routes that say so
        const bool rounded = r.rounded_bias || r.kernel == GG_ATTN_KERNEL_BWD || r.kernel == GG_ATTN_KERNEL_BWD_GROUPED;
        return gg_attention_dbias(&db, attn_dtype(e.f32), rounded, e.st);
    }
    if (at.dbias && gg_attention_route(&at, attn_entry(e.f32, e.attn16, e.attn16_train, at, true), attn_dtype(e.f32), &r) == 0 &&
        r.dbias_rows * st.heads * st.ws * st.ws * 4 <= ((int64_t)64 << 20))
        at.dbias_scratch = e.F(L.splitk);
    if (e.f32 && L.attn_ds >= 0 && !attn_switches().no_ds_scratch) at.ds_scratch = e.F(L.attn_ds);
    return attention_run(e, at, true);
}
// padded block: zero-pad a [B, res, res, C] map of the stage to [B, pres, pres, C]; crop such a map back: y = res_in + rowscale[b] * t (y may be res_in)
static int window_pad(const Exec& e, const StageL& st, const act_t* x, act_t* y) {
    return gg_window_pad(x, y, e.B, st.res, st.res, st.pres, st.pres, st.C, e.f32 ? 1 : 0, e.st);
}
static int window_crop_add(const Exec& e, const StageL& st, const act_t* t, const act_t* res_in, const float* rowscale, act_t* y) {
    return gg_window_crop_add(t, res_in, rowscale, y, e.B, st.res, st.res, st.pres, st.pres, st.C, e.f32 ? 1 : 0, e.st);
}
// the padded input of LayerNorm1 survives into the backward (its own storage, or the segment region under recompute) unless neither LayerNorm1 nor qkv trains
static bool xpad_kept(const Exec& e, const BlockL& l) { return e.m->cfg.recompute || e.tr(l.qkv.t_w) || e.tr(l.ln1.t_g); }
// PatchEmbed's gathers: the f32 NCHW image -> col1 [B*(H/2)^2, 32]; act(BN(y)) of an NHWC ConvNorm -> col [B*(H/2)^2, 9 C] (the activation is never written)
static int im2col_image(const Exec& e, const float* x, act_t* col, int B, int H, int W) {
    if (e.f32) return gg_im2col_nchw3_f32_f32(x, (float*)col, B, H, W, 2, e.st);
    return gg_im2col_nchw3_f32(x, col, B, H, W, 2, e.st);
}
static int im2col_bn(const Exec& e, const BNP& bn, const Act& a, int act, act_t* col, int B, int H, int W) {
    if (e.f32) return gg_im2col_nhwc_f32((const float*)e.A(a.y), e.F(a.stat), e.P(bn.t_g), e.P(bn.t_b), act, (float*)col, B, H, W, bn.C, 2, e.st);
    return gg_im2col_nhwc_bn_bf16(e.A(a.y), e.F(a.stat), e.P(bn.t_g), e.P(bn.t_b), act, col, B, H, W, bn.C, 2, e.st);
}
static int token_mean_fwd(const Exec& e, const act_t* x, float* pooled, int B, int T, int C) {
    return e.f32 ? gg_token_mean_fwd_f32((const float*)x, pooled, B, T, C, e.st) : gg_token_mean_fwd(x, pooled, B, T, C, e.st);
}
static int token_mean_bwd(const Exec& e, const float* dpool, act_t* dx, int B, int T, int C) {
    return e.f32 ? gg_token_mean_bwd_f32(dpool, (float*)dx, B, T, C, e.st) : gg_token_mean_bwd(dpool, dx, B, T, C, e.st);
}

// ------------------------------------------------------------------------------------------- forward
// One segment each: an MBConv of stage 0, a PatchMerging, a TinyVitBlock.  forward_impl runs them in order; under activation recompute
// (GgTinyVitCfg.recompute = 1) backward_impl runs each again with e.replay right before the segment's backward: the same launches on the same
// routes (fusion flags, split routing, the trainable-mask conditions), minus the segment's last launch -- the one that writes its output
// checkpoint, which the segment's backward does not read -- and with no BatchNorm finalisation (bn_stats).
// (the output of everything in front of stages[s]; s = 3: the last feature map, the head's input)
static int64_t merge_input(const Layout& L, int s) {
    return s == 0 ? (L.mb.empty() ? L.x_pe : L.mb.back().out) : (L.blocks[s - 1].empty() ? L.merge[s - 1].out : L.blocks[s - 1].back().x3);
}
static int mbconv_fwd(const Exec& e, size_t i, int slot) {
    const Model& m = *e.m; const GgTinyVitCfg& c = m.cfg;
    const int* d = c.embed_dims;
    const int B = e.B, H0 = m.res0;
    const int64_t M0 = (int64_t)B * H0 * H0;
    const int mid = (int)(d[0] * c.mbconv_expand_ratio);
    const MBConvL& l = m.mb[i]; const MBAct& a = e.L->mb[i];
    GG_TRY(conv_dense_fwd(e, l.c1, a.c1, e.A(a.x), d[0], M0));
    if (act1_fused_away(e.sch(), 1)) {
        GG_TRY(conv_dw_fwd_fused(e, l.c2, a.c2, l.c1.bn, a.c1, GG_ACT_GELU, B, H0, H0, 1));   // act1 is never materialised
    } else {
        GG_TRY(bn_apply(e, l.c1.bn, a.c1, M0, GG_ACT_GELU, e.A(a.a1)));
        GG_TRY(conv_dw_fwd(e, l.c2, a.c2, e.A(a.a1), B, H0, H0, 1));
    }
    if (conv3_takes_prologue(e.sch(), l.c3.w, mid, e.training && e.tr(l.c3.w.t_w))) {
        GG_TRY(conv_dense_fwd_pro(e, l.c3, a.c3, l.c2.bn, a.c2, GG_ACT_GELU, M0));
    } else {
        GG_TRY(bn_apply(e, l.c2.bn, a.c2, M0, GG_ACT_GELU, e.A(a.a2)));
        GG_TRY(conv_dense_fwd(e, l.c3, a.c3, e.A(a.a2), mid, M0));
    }
    if (e.replay) return 0;
    return bn_apply(e, l.c3.bn, a.c3, M0, GG_ACT_GELU, e.A(a.out), e.A(a.x), e.training ? e.dropv(slot) : nullptr, H0 * H0);
}
static int merge_fwd(const Exec& e, int s) {
    const Model& m = *e.m; const Layout& L = *e.L;
    const int B = e.B;
    const StageL& st = m.stages[s];
    const int C = st.C;
    const int res = s == 0 ? m.res0 : m.stages[s - 1].res, Cprev = s == 0 ? m.cfg.embed_dims[0] : m.stages[s - 1].C;
    const int64_t M = (int64_t)B * st.res * st.res, Mprev = (int64_t)B * res * res;
    const MergeAct& ma = L.merge[s];
    GG_TRY(conv_dense_fwd(e, st.merge.c1, ma.c1, e.A(merge_input(L, s)), Cprev, Mprev));
    if (act1_fused_away(e.sch(), 2)) {
        GG_TRY(conv_dw_fwd_fused(e, st.merge.c2, ma.c2, st.merge.c1.bn, ma.c1, GG_ACT_GELU, B, res, res, 2));
    } else {
        GG_TRY(bn_apply(e, st.merge.c1.bn, ma.c1, Mprev, GG_ACT_GELU, e.A(ma.a1)));
        GG_TRY(conv_dw_fwd(e, st.merge.c2, ma.c2, e.A(ma.a1), B, res, res, 2));
    }
    GG_TRY(bn_apply(e, st.merge.c2.bn, ma.c2, M, GG_ACT_GELU, e.A(ma.a2)));
    GG_TRY(conv_dense_fwd(e, st.merge.c3, ma.c3, e.A(ma.a2), C, M));
    if (e.replay) return 0;
    return bn_apply(e, st.merge.c3.bn, ma.c3, M, GG_ACT_NONE, e.A(ma.out));
}
// DropPath row compaction.  A dropped sample's branch is multiplied by zero in forward and receives a zero gradient in backward; in a block that
// qualifies the kept samples' rows are compacted (row r <-> physical row kept[r / rps] * rps + r % rps) and the MLP branch -- forward and backward -- and the backward
// of the attention branch run over them only.  The attention branch's FORWARD still covers every sample in map order (its output is a tap of the block).
// A block qualifies when: fp32_split training with a drop array; it is a stage-2 block of width >= 384 with one window per image; every parameter of it is frozen (no weight,
// bias, LayerNorm / BatchNorm or attention-bias gradient reads a branch tensor); the fused norm2 forms are on; and all eight Linear launches (four forward, four data
// gradients) take the 256 x 128 split GEMM.  Forward, recompute replay and backward evaluate this from the same inputs.
// The kept lists (count, kept sample indices in ascending order, each sample's compact position) are derived on the device from the caller's scales -- kept <=> scale != 0 --
// by one small launch in front of the block's forward, replay and backward (block_lists); no host synchronisation: grids are sized for all rows and read the count.
// A padded block (pres != res: the window does not divide the map) never compacts: one window per image means res == ws, and such a map is not padded.
static bool block_compacts(const Exec& e, int s, size_t i) {
    const Model& m = *e.m; const Schedule& k = m.sch;
    const StageL& st = m.stages[s];
    const BlockL& l = st.blocks[i];
    const int C = st.C, hid = (int)(C * m.cfg.mlp_ratio), rps = st.res * st.res;
    const int64_t M = (int64_t)e.B * rps;
    if (!e.compact || !m.split || !e.training || !e.drop || !e.trainable || (int64_t)2 * gg_drop_list_ints(e.B) * 4 > e.L->colsum_bytes) return false;
    if (s != 1 || C < 384 || C > 640 || st.res != st.ws || st.pres != st.res || M * hid * 4 >= ((int64_t)1 << 31)) return false;
    for (int t : {l.t_ab, l.ln1.t_g, l.ln1.t_b, l.qkv.t_w, l.qkv.t_b, l.proj.t_w, l.proj.t_b, l.ln2.t_g, l.ln2.t_b, l.fc1.t_w, l.fc1.t_b, l.fc2.t_w, l.fc2.t_b,
                  l.local.w.t_w, l.local.bn.t_g, l.local.bn.t_b})
        if (e.tr(t)) return false;
    if (!(k.fuse_lnbn && k.fuse_lncol && k.fuse_bnbwd)) return false;
    {   // the attention backward must take the window map: one route does (the single-pass split kernel: 14 x 14, 12 x 12, 7 x 7 windows), every other refuses it
        GgAttnArgs at;
        GgAttnRoute r;
        attn_shape(st, e.B, at);
        at.dout = at.qkv; at.lddo = at.ldo; at.dqkv = at.out; at.window_map = at.num_windows_dev = (const int*)at.qkv;
        if (gg_attention_route(&at, GG_ATTN_ENTRY_FLASH_BWD, 1, &r) != 0) return false;
    }
    struct Lin { const DenseW* w; bool t; int N, K; };
    const Lin lins[8] = {{&l.qkv, false, 3 * C, l.qkv.Kp}, {&l.proj, false, C, l.proj.Kp}, {&l.fc1, false, hid, l.fc1.Kp}, {&l.fc2, false, C, l.fc2.Kp},
                         {&l.fc2, true, hid, C}, {&l.fc1, true, C, hid}, {&l.proj, true, C, C}, {&l.qkv, true, C, 3 * C}};
    for (const Lin& x : lins) {
        const int64_t tiles = ((M + 255) / 256) * ((x.N + 127) / 128);
        if (x.K < 384 || (x.K & 7) || tiles < split_min_tiles() || !gg_split3_af32_takes_rowmap(x.N, x.K)) return false;
        if (!planes_of(e, x.t ? e.Wt(*x.w) : e.Wn(*x.w), x.t ? x.w->Np : x.w->Kp, x.N)) return false;
    }
    return true;
}
static int block_lists(const Exec& e, int slot) { return gg_drop_kept_lists(e.dropv(slot), 2, e.B, e.drop_list(0), e.st); }
static int block_fwd(const Exec& e, int s, size_t i, int slot) {
    const Model& m = *e.m; const GgTinyVitCfg& c = m.cfg;
    const int B = e.B;
    const StageL& st = m.stages[s];
    const int C = st.C;
    const int64_t M = (int64_t)B * st.res * st.res;
    const int hid = (int)(C * c.mlp_ratio);
    const int rps = st.res * st.res;
    const BlockL& l = st.blocks[i]; const BlockAct& a = e.L->blocks[s][i];
    const float* s1 = e.training ? e.dropv(slot) : nullptr;
    const float* s2 = e.training ? e.dropv(slot + 1) : nullptr;
    const bool compacts = block_compacts(e, s, i);
    if (compacts) GG_TRY(block_lists(e, slot));
    // padded block (the window does not divide the map): x0 is zero-padded in front of LayerNorm1 -- a pad token leaves the norm as norm.bias and takes part in its
    // window as key and value, nothing masks it -- the branch runs at Mp rows, and proj's result is cropped back where the residual is added
    const bool padded = st.pres != st.res;
    const int64_t Mp = (int64_t)B * st.pres * st.pres;
    if (padded) GG_TRY(window_pad(e, st, e.A(a.x0), e.A(a.xpad)));
    GG_TRY(gg_layernorm_fwd(e.A(padded ? a.xpad : a.x0), e.f32, e.P(l.ln1.t_g), e.P(l.ln1.t_b), Mp, C, c.ln_eps, e.A(a.a), e.f32, e.F(a.mean1), e.F(a.rstd1), e.st));
    GG_TRY(gemm(e, e.A(a.a), C, e.Wn(l.qkv), l.qkv.Kp, e.A(a.qkv), 3 * C, Mp, 3 * C, l.qkv.Kp, e.P(l.qkv.t_b)));
    GgAttnArgs at;
    attn_args(e, st, l, a, B, at);
    GG_TRY(attention_fwd(e, at));
    if (padded) {
        GG_TRY(gemm(e, e.A(a.o), C, e.Wn(l.proj), l.proj.Kp, e.A(e.L->padtmp), C, Mp, C, l.proj.Kp, e.P(l.proj.t_b)));
        GG_TRY(window_crop_add(e, st, e.A(e.L->padtmp), e.A(a.x0), s1, e.A(a.x1)));
    } else {
        GG_TRY(gemm(e, e.A(a.o), C, e.Wn(l.proj), l.proj.Kp, e.A(a.x1), C, M, C, l.proj.Kp, e.P(l.proj.t_b), 0, nullptr, s1, rps, e.A(a.x0)));
    }
    GG_TRY(conv_dw_fwd(e, l.local, a.local, e.A(a.x1), B, st.res, st.res, 1));
    if (compacts) {
        // MLP branch over the kept samples' rows: norm2 writes x2 for every row, `b` compact, and the block's output x3 := x2 for the dropped samples (not in a replay:
        // x3 is the checkpoint); fc1 runs compact to compact; fc2's residual epilogue reads x2 and writes x3 through the row map
        const int* list = e.drop_list(1);
        const RowMap cc = {list, rps, false, false}, out = {list, rps, false, true};
        GG_TRY(gg_layernorm_fwd_bn_f32_map((const float*)e.A(a.local.y), e.F(a.local.stat), e.P(l.local.bn.t_g), e.P(l.local.bn.t_b), (float*)e.A(a.x2), e.P(l.ln2.t_g),
                                           e.P(l.ln2.t_b), M, C, c.ln_eps, (float*)e.A(a.b), e.F(a.mean2), e.F(a.rstd2), list + GG_DROP_LIST_HEAD + B, rps,
                                           e.replay ? nullptr : (float*)e.A(a.x3), e.st));
        GG_TRY(gemm(e, e.A(a.b), C, e.Wn(l.fc1), l.fc1.Kp, e.A(a.h), hid, M, hid, l.fc1.Kp, e.P(l.fc1.t_b), GG_ACT_GELU, (void*)e.A(a.hpre), nullptr, 0, nullptr, nullptr,
                    nullptr, 0, &cc));
        if (e.replay) return 0;
        return gemm(e, e.A(a.h), hid, e.Wn(l.fc2), l.fc2.Kp, e.A(a.x3), C, M, C, l.fc2.Kp, e.P(l.fc2.t_b), 0, nullptr, s2, rps, e.A(a.x2), nullptr, nullptr, 0, &out);
    }
    if (C <= 640 && e.f32 && e.sch().fuse_lnbn) {     // BatchNorm apply of local_conv rides on norm2's load (x2 = the residual stream is written there)
        GG_TRY(gg_layernorm_fwd_bn_f32((const float*)e.A(a.local.y), e.F(a.local.stat), e.P(l.local.bn.t_g), e.P(l.local.bn.t_b), (float*)e.A(a.x2),
                                       e.P(l.ln2.t_g), e.P(l.ln2.t_b), M, C, c.ln_eps, (float*)e.A(a.b), e.F(a.mean2), e.F(a.rstd2), e.st));
    } else if (C <= 640 && !e.f32) {
        GG_TRY(gg_layernorm_fwd_bn(e.A(a.local.y), e.F(a.local.stat), e.P(l.local.bn.t_g), e.P(l.local.bn.t_b), e.A(a.x2), e.P(l.ln2.t_g),
                                   e.P(l.ln2.t_b), M, C, c.ln_eps, e.A(a.b), e.F(a.mean2), e.F(a.rstd2), e.st));
    } else {
        GG_TRY(bn_apply(e, l.local.bn, a.local, M, GG_ACT_NONE, e.A(a.x2)));
        GG_TRY(gg_layernorm_fwd(e.A(a.x2), e.f32, e.P(l.ln2.t_g), e.P(l.ln2.t_b), M, C, c.ln_eps, e.A(a.b), e.f32, e.F(a.mean2), e.F(a.rstd2), e.st));
    }
    GG_TRY(gemm(e, e.A(a.b), C, e.Wn(l.fc1), l.fc1.Kp, e.A(a.h), hid, M, hid, l.fc1.Kp, e.P(l.fc1.t_b), GG_ACT_GELU,
                e.training ? (void*)e.A(a.hpre) : nullptr));
    if (e.replay) return 0;
    return gemm(e, e.A(a.h), hid, e.Wn(l.fc2), l.fc2.Kp, e.A(a.x3), C, M, C, l.fc2.Kp, e.P(l.fc2.t_b), 0, nullptr, s2, rps, e.A(a.x2));
}

static int segment_fwd(const Exec& e, const Segment& sg) {
    if (sg.kind == SEG_MBCONV) return mbconv_fwd(e, (size_t)sg.index, sg.slot);
    return sg.kind == SEG_MERGE ? merge_fwd(e, sg.stage - 1) : block_fwd(e, sg.stage - 1, (size_t)sg.index, sg.slot);
}
// PatchEmbed: conv3x3 s2 + BN + GELU, conv3x3 s2 + BN
static int patch_embed_fwd(const Exec& e, const float* x) {
    const Model& m = *e.m; const Layout& L = *e.L;
    const int B = e.B, H = m.cfg.img_size, H1 = H / 2, H0 = m.res0;
    const int64_t M1 = (int64_t)B * H1 * H1, M0 = (int64_t)B * H0 * H0;
    GG_TRY(im2col_image(e, x, e.A(L.col1), B, H, H));
    GG_TRY(conv_dense_fwd(e, m.pe1, L.pe1, e.A(L.col1), 32, M1));
    GG_CHECK(m.pe2.w.Kp == m.pe2.w.K, "tinyvit: patch_embed.conv2 K=%d must be a multiple of 8", m.pe2.w.K);
    // BN1 + GELU ride on conv2's im2col gather: the activation tensor (M1 x 48, the largest of the model) is never written
    GG_TRY(im2col_bn(e, m.pe1.bn, L.pe1, GG_ACT_GELU, e.A(L.col2), B, H1, H1));
    GG_TRY(conv_dense_fwd(e, m.pe2, L.pe2, e.A(L.col2), m.pe2.w.Kp, M0));
    return bn_apply(e, m.pe2.bn, L.pe2, M0, GG_ACT_NONE, e.A(L.x_pe));
}
// head: global average pool -> LayerNorm
static int head_fwd(const Exec& e, float* out) {
    const Model& m = *e.m; const Layout& L = *e.L; const GgTinyVitCfg& c = m.cfg;
    const int B = e.B, res = m.stages[2].res, T = res * res, C3 = c.embed_dims[3];
    GG_TRY(token_mean_fwd(e, e.A(merge_input(L, 3)), e.F(L.pooled), B, T, C3));
    if (c.features_only) {     // models/tinyvit.py:139-143: the pooled last feature map, no head.norm
        GG_HIP(hipMemcpyAsync(out, e.F(L.pooled), (size_t)B * C3 * sizeof(float), hipMemcpyDeviceToDevice, e.st));
        return 0;
    }
    return gg_layernorm_fwd(e.F(L.pooled), 1, e.P(m.head.t_g), e.P(m.head.t_b), B, C3, c.ln_eps, out, 1, e.F(L.mean_h), e.F(L.rstd_h), e.st);
}
// (num_batches_tracked counters are bumped by the host shim: they are int64 bookkeeping, not arithmetic)
static int forward_impl(const Exec& e, const float* x, float* out) {
    GG_TRY(patch_embed_fwd(e, x));
    for (const Segment& sg : e.m->segs) GG_TRY(segment_fwd(e, sg));
    return head_fwd(e, out);
}

// BatchNorm-backward pieces on the shared scratch: partial rows at the start of `bnscratch`, coef [3][C] right behind them
static float* bn_coef(const Exec& e, int64_t M, int C) { return e.F(e.L->bnscratch) + ((int64_t)gg_bn_bwd_rows(M, C) + GG_REDUCE_SLICES) * 2 * C; }
// finalize the BatchNorm-backward sums in `rows` partial rows at `part`: coef -> bn_coef(e, M, C), the parameter gradients if they train
static int bn_bwd_fin(const Exec& e, const BNP& bn, const Act& a, int64_t M, float* part, int rows) {
    const bool tr = e.tr(bn.t_g);
    return gg_bn_bwd_finalize(part, rows, bn.C, M, e.F(a.stat), e.P(bn.t_g), bn_coef(e, M, bn.C), tr ? e.Gd(bn.t_g) : nullptr,
                              tr ? e.Gd(bn.t_b) : nullptr, 1, e.st);
}
static int bn_bwd_reduce_fin(const Exec& e, const BNP& bn, const Act& a, int64_t M, int act, const act_t* dout, act_t* dz) {
    if (e.f32) GG_TRY(gg_bn_bwd_reduce_f32((const float*)dout, (const float*)e.A(a.y), e.F(a.stat), e.P(bn.t_g), e.P(bn.t_b), M, bn.C, act, nullptr,
                                           nullptr, 0, (float*)dz, e.F(e.L->bnscratch), e.st));
    else GG_TRY(gg_bn_bwd_reduce(dout, e.A(a.y), e.F(a.stat), e.P(bn.t_g), e.P(bn.t_b), M, bn.C, act, nullptr, nullptr, 0, dz,
                            e.F(e.L->bnscratch), e.st));
    return bn_bwd_fin(e, bn, a, M, e.F(e.L->bnscratch), gg_bn_bwd_rows(M, bn.C));
}
// conv dgrad with the BatchNorm-backward reduce of the ConvNorm it feeds as epilogue: dz = (dY . W) * act'(BN(y)), partial
// column sums -> statpart, then their finalize
static int gemm_bnbwd(const Exec& e, const act_t* dY, int64_t ldy, const act_t* Wt, int64_t ldw, act_t* dz, int64_t M, int N, int K,
                      const BNP& bn, const Act& a, int act) {
    GgGemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = dY; g.lda = ldy; g.B = Wt; g.ldb = ldw; g.C = dz; g.ldc = N; g.M = (int)M; g.N = N; g.K = K;
    g.bn_y = e.A(a.y); g.bn_stat = e.F(a.stat); g.bn_gamma = e.P(bn.t_g); g.bn_beta = e.P(bn.t_b); g.bn_act = act;
    g.colstats = e.F(e.L->statpart);
    GG_TRY(e.f32 ? gg_gemm_nt_f32(&g, e.st) : gg_gemm_nt(&g, e.st));
    return bn_bwd_fin(e, bn, a, M, e.F(e.L->statpart), gg_gemm_colstats_rows((int)M));
}

__global__ void conv_wgrad_scatter_kernel(const float* __restrict__ src, int N, int Kp, int cin, int taps, float* __restrict__ grad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // over N * cin * taps (grad layout (co, ci, tap))
    if (i >= N * cin * taps) return;
    const int tap = i % taps, ci = (i / taps) % cin, co = i / (taps * cin);
    grad[i] += src[(int64_t)co * Kp + tap * cin + ci];
}
static int conv_wgrad_scatter(const float* src, int N, int Kp, int cin, int taps, float* grad, hipStream_t st) {
    const int n = N * cin * taps;
    hipLaunchKernelGGL(conv_wgrad_scatter_kernel, dim3((unsigned)gg_cdiv(n, 256)), dim3(256), 0, st, src, N, Kp, cin, taps, grad);
    GG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------- backward helpers
// wgrad of a dense weight: dW[N,K] (+)= dY^T[N,M] . X[M,K]   (transposes into scratch, split-K over M)
static int dense_wgrad(const Exec& e, const DenseW& w, const act_t* X, int64_t ldx, const act_t* dY, int64_t ldy, int64_t M,
                       const float* rowscale, int rps, bool conv_reorder) {
    const int K = conv_reorder ? w.Kp : w.K;   // im2col'd operand has Kp columns
    // fp32_split mode: the weight gradient of a block Linear (the tensors that have planes) as split products too, same slab protocol
    static const char* tn_min_env = gg_dev_env("GG_SPLIT_TN_MIN_M");      // (dev: the same for the weight gradients' row threshold)
    static const int64_t tn_min_m = tn_min_env ? atoll(tn_min_env) : 1024;
    const bool sp = e.m->split && w.wn3 >= 0 && !conv_reorder && M >= tn_min_m;
    // ... and that of a dense convolution whose whole output fits one workgroup (patch_embed.conv2: 96 x 432) on the resident form, from the row count at which
    // its one-workgroup-per-slab grid fills the chip (256 slabs of 8 stages); below it, and for every larger output, gg_gemm_tn_f32 as before
    const char* res_min_env = gg_dev_env("GG_SPLIT_TN_RESIDENT_MIN_M");      // (dev: the resident form's row threshold; read per call, so that one process can
    const int64_t res_min_m = res_min_env ? atoll(res_min_env) : 65536;      // compare both routes -- tools/patch_embed_bwd_check.py)
    const bool res = e.m->split && e.f32 && conv_reorder && M >= res_min_m && gg_gemm_tn_split3_resident_fits(w.N, K) != 0;
    const int split = res ? gg_gemm_tn_split3_resident_splits((int)M, w.N, K) :
                      sp ? gg_gemm_tn_split3_splits((int)M, w.N, K) : e.f32 ? gg_gemm_tn_f32_splits((int)M, w.N, K) : gg_gemm_tn_splits((int)M, w.N, K);
    if (res) {
        GG_CHECK(split > 0, "dense_wgrad: no slab count for the resident weight gradient");
        GG_TRY(gg_gemm_tn_split3_resident((const float*)dY, ldy, (const float*)X, ldx, (int)M, w.N, K, e.F(e.L->splitk), split, e.st));
    } else if (sp) GG_TRY(gg_gemm_tn_split3((const float*)dY, ldy, (const float*)X, ldx, (int)M, w.N, K, rowscale, rps, e.F(e.L->splitk), split, e.st));
    else if (e.f32) GG_TRY(gg_gemm_tn_f32(dY, ldy, X, ldx, (int)M, w.N, K, rowscale, rps, e.F(e.L->splitk), split, e.st));
    else GG_TRY(gg_gemm_tn(dY, ldy, X, ldx, (int)M, w.N, K, rowscale, rps, e.F(e.L->splitk), split, e.st));
    float* gw = e.Gd(w.t_w);
    if (!conv_reorder) {
        GG_TRY(gg_splitk_reduce(e.F(e.L->splitk), gw, (int64_t)w.N * K, split, 1, 1.0f, e.st));
    } else {
        // reduce in place, then scatter (co,(ky,kx,ci)) -> (co,ci,ky,kx)
        GG_TRY(gg_splitk_reduce(e.F(e.L->splitk), e.F(e.L->splitk), (int64_t)w.N * K, split, 0, 1.0f, e.st));
        GG_TRY(conv_wgrad_scatter(e.F(e.L->splitk), w.N, K, w.cin, w.taps, gw, e.st));
    }
    return 0;
}
// PatchEmbed conv2's col2im (stride 2, onto conv1's [B, H, W] map): plain, and with the BatchNorm-backward reduce of conv1's ConvNorm riding on it
static int col2im(const Exec& e, const act_t* dcol, act_t* dx, int B, int H, int W, int C) {
    if (e.f32) return gg_col2im_nhwc_f32((const float*)dcol, (float*)dx, B, H, W, C, 2, e.st);
    return gg_col2im_nhwc_bf16(dcol, dx, B, H, W, C, 2, e.st);
}
static int col2im_bnbwd(const Exec& e, const act_t* dcol, const BNP& bn, const Act& a, int act, act_t* dz, int nparts, int B, int H, int W) {
    if (e.f32) return gg_col2im_nhwc_bnbwd_f32((const float*)dcol, (const float*)e.A(a.y), e.F(a.stat), e.P(bn.t_g), e.P(bn.t_b), act, (float*)dz,
                                               e.F(e.L->bnscratch), nparts, B, H, W, bn.C, e.st);
    return gg_col2im_nhwc_bnbwd_bf16(dcol, e.A(a.y), e.F(a.stat), e.P(bn.t_g), e.P(bn.t_b), act, dz, e.F(e.L->bnscratch), nparts, B, H, W, bn.C, e.st);
}
// weight gradient of a ConvNorm whose dy feeds nothing else (the first conv of the network): BatchNorm backward stops after
// reduce + finalize, and the TN GEMM forms dy = c0*dz + c1*y + c2 from (dz, y) while loading -- no apply pass, no dy tensor
// The output gradient does not exist yet either: the reduce rides on the col2im that would have produced it from dcol ([B, H, W] map, stride 2).
// `next` (fp32_split): no dcol -- the stride-2 convolution `next` behind this ConvNorm hands over its output gradient dy_next and the data gradient is formed by input
// parity in the same launch (gg_conv3x3s2_dgrad_bnbwd_split3; `dcol` is then its plane scratch)
static int convnorm_wgrad_from_dz(const Exec& e, const ConvBNDense& c, const Act& a, int64_t M, int act, act_t* dz, const act_t* X, int64_t ldx,
                                  const act_t* dcol, int B, int H, int W, const ConvBNDense* next = nullptr, const act_t* dy_next = nullptr) {
    const BNP& bn = c.bn; const DenseW& w = c.w;
    const int nb = std::min(gg_bn_bwd_rows(M, bn.C), 65535), K = w.Kp;
    if (next) GG_TRY(gg_conv3x3s2_dgrad_bnbwd_split3((const float*)dy_next, (const float*)e.Wt(next->w), next->w.Np, (const float*)e.A(a.y), e.F(a.stat), e.P(bn.t_g), e.P(bn.t_b),
                                                     act, (float*)dz, e.F(e.L->bnscratch), nb, (void*)dcol, B, H, W, bn.C, next->w.N, e.st));
    else GG_TRY(col2im_bnbwd(e, dcol, bn, a, act, dz, nb, B, H, W));
    GG_TRY(bn_bwd_fin(e, bn, a, M, e.F(e.L->bnscratch), nb));
    if (!e.tr(w.t_w)) return 0;
    const int split = e.f32 ? gg_gemm_tn_f32_splits((int)M, w.N, K) : gg_gemm_tn_splits((int)M, w.N, K);
    if (e.f32) GG_TRY(gg_gemm_tn_bn_f32(dz, e.A(a.y), bn.C, bn_coef(e, M, bn.C), X, ldx, (int)M, w.N, K, e.F(e.L->splitk), split, e.st));
    else GG_TRY(gg_gemm_tn_bn(dz, e.A(a.y), bn.C, bn_coef(e, M, bn.C), X, ldx, (int)M, w.N, K, e.F(e.L->splitk), split, e.st));
    GG_TRY(gg_splitk_reduce(e.F(e.L->splitk), e.F(e.L->splitk), (int64_t)w.N * K, split, 0, 1.0f, e.st));
    return conv_wgrad_scatter(e.F(e.L->splitk), w.N, K, w.cin, w.taps, e.Gd(w.t_w), e.st);
}
static int bias_grad(const Exec& e, int t_b, const act_t* dY, int64_t ld, int64_t M, int N, const float* rowscale, int rps) {
    if (e.f32) return gg_colsum_f32((const float*)dY, ld, (int)M, N, rowscale, rps, e.F(e.L->colsum), e.Gd(t_b), 1, e.st);
    return gg_colsum_bf16(dY, ld, (int)M, N, rowscale, rps, e.F(e.L->colsum), e.Gd(t_b), 1, e.st);
}
// BatchNorm backward of one ConvNorm: dout (grad wrt post-activation output) -> dy (grad wrt the conv output)
static int bn_bwd(const Exec& e, const BNP& bn, const Act& a, int64_t M, int act, const act_t* dout, act_t* dz, act_t* dy,
                  const act_t* residual = nullptr, const float* rowscale = nullptr, int rps = 0) {
    const bool tr = e.tr(bn.t_g);
    if (e.f32) return gg_bn_bwd_f32((const float*)dout, (const float*)e.A(a.y), e.F(a.stat), e.P(bn.t_g), e.P(bn.t_b), M, bn.C, act,
                                    (const float*)residual, rowscale, rps, (float*)dz, (float*)dy, e.F(e.L->bnscratch),
                                    tr ? e.Gd(bn.t_g) : nullptr, tr ? e.Gd(bn.t_b) : nullptr, 1, e.st);
    return gg_bn_bwd(dout, e.A(a.y), e.F(a.stat), e.P(bn.t_g), e.P(bn.t_b), M, bn.C, act, residual, rowscale, rps, dz, dy,
                     e.F(e.L->bnscratch), tr ? e.Gd(bn.t_g) : nullptr, tr ? e.Gd(bn.t_b) : nullptr, 1, e.st);
}

static int bn_bwd_apply_only(const Exec& e, const act_t* dz, const act_t* y, const float* coef, int64_t M, int C, act_t* dy) {
    if (e.f32) return gg_bn_bwd_apply_f32((const float*)dz, (const float*)y, coef, M, C, nullptr, 0, (float*)dy, e.st);
    return gg_bn_bwd_apply(dz, y, coef, M, C, nullptr, 0, dy, e.st);
}
// stride-1 depthwise data gradient with the BatchNorm-backward fusions on its input (apply) and output (reduce) sides
static int dw_bwd_data_fused(const Exec& e, const act_t* dz_in, const act_t* y_in, const float* in_coef, const DwW& w, act_t* out, int B, int H, int W,
                             const act_t* ep_y, const float* ep_stat, const float* ep_gamma, const float* ep_beta, int ep_act, float* ep_part) {
    if (e.f32) return gg_dwconv3x3_bwd_data_fused_f32((const float*)dz_in, (const float*)y_in, in_coef, e.Taps(w), (float*)out, B, H, W, w.C,
                                                      (const float*)ep_y, ep_stat, ep_gamma, ep_beta, ep_act, ep_part, e.st);
    return gg_dwconv3x3_bwd_data_fused(dz_in, y_in, in_coef, e.Taps(w), out, B, H, W, w.C, ep_y, ep_stat, ep_gamma, ep_beta, ep_act, ep_part, e.st);
}
// The fused depthwise data gradient (stride 1: MBConv, 2: PatchMerging; [B, H, W] = the conv's input map) with its epilogue on, then the finalize of the
// BatchNorm in front (bn1 / a1): dz1 = da1 * GELU'(BN1(y1)) -> dz1, BN1's backward sums -> statpart -> coef at bn_coef(e, B*H*W, C) and BN1's parameter
// gradients.  The conv's own input dy2 is formed at its taps from (dz_in, y_in, in_coef), or is dz_in as given (y_in = in_coef = null; stride 1 only).
static int dw_bwd_data_fused_fin(const Exec& e, const DwW& w, const act_t* dz_in, const act_t* y_in, const float* in_coef, act_t* dz1, int B, int H, int W,
                                 int stride, const BNP& bn1, const Act& a1) {
    const int C = w.C;
    int rows;
    if (stride == 1) {
        GG_TRY(dw_bwd_data_fused(e, dz_in, y_in, in_coef, w, dz1, B, H, W, e.A(a1.y), e.F(a1.stat), e.P(bn1.t_g), e.P(bn1.t_b), GG_ACT_GELU, e.F(e.L->statpart)));
        rows = e.f32 ? gg_dwconv_f32_stat_rows(B, H, W, C, 1) : gg_dwconv_fused_stat_rows(B, H, W, C, in_coef != nullptr);
    } else if (e.f32) {
        GG_TRY(gg_dwconv3x3_s2_bwd_data_fused_f32((const float*)dz_in, (const float*)y_in, in_coef, e.Taps(w), (float*)dz1, B, H, W, C, (const float*)e.A(a1.y),
                                                  e.F(a1.stat), e.P(bn1.t_g), e.P(bn1.t_b), GG_ACT_GELU, e.F(e.L->statpart), e.st));
        rows = gg_dwconv_f32_s2_fused_stat_rows(B, H, W, C);
    } else {
        GG_TRY(gg_dwconv3x3_s2_bwd_data_fused(dz_in, y_in, in_coef, e.Taps(w), dz1, B, H, W, C, e.A(a1.y), e.F(a1.stat), e.P(bn1.t_g), e.P(bn1.t_b),
                                              GG_ACT_GELU, e.F(e.L->statpart), e.st));
        rows = gg_dwconv_s2_fused_stat_rows(B, H, W, C);
    }
    return bn_bwd_fin(e, bn1, a1, (int64_t)B * H * W, e.F(e.L->statpart), rows);
}
static int dw_bwd_data(const Exec& e, const DwW& w, const act_t* dy, act_t* dx, int B, int H, int W, int stride) {
    if (e.f32) return gg_dwconv3x3_bwd_data_f32((const float*)dy, e.Taps(w), (float*)dx, B, H, W, w.C, stride, e.st);
    return gg_dwconv3x3_bwd_data(dy, e.Taps(w), dx, B, H, W, w.C, stride, e.st);
}
static int dw_bwd_weight(const Exec& e, const DwW& w, const act_t* x, const act_t* dy, int B, int H, int W, int stride) {
    if (e.f32) return gg_dwconv3x3_bwd_weight_f32((const float*)x, (const float*)dy, B, H, W, w.C, stride, e.F(e.L->bnscratch), e.Gd(w.t_w), 1, e.st);
    return gg_dwconv3x3_bwd_weight(x, dy, B, H, W, w.C, stride, e.F(e.L->bnscratch), e.Gd(w.t_w), 1, e.st);
}
// tap gradient of conv2 of an MBConv / a PatchMerging, whose input is act1 = GELU(BN1(y1)): re-formed here first where the forward never wrote it
static int dw_bwd_weight_act1(const Exec& e, const DwW& w, const BNP& bn1, const Act& a1, int64_t act1, const act_t* dy, int B, int H, int W, int stride) {
    if (act1_fused_away(e.sch(), stride)) GG_TRY(bn_apply(e, bn1, a1, (int64_t)B * H * W, GG_ACT_GELU, e.A(act1)));
    return dw_bwd_weight(e, w, e.A(act1), dy, B, H, W, stride);
}

// ------------------------------------------------------------------------------------------- backward
// One function per segment, mirroring the forward's.  The five gradient buffers (scratch.G0..G4): dx holds the gradient w.r.t. the segment's output
// when its backward starts and w.r.t. its input when it returns; a..d are temporaries that carry nothing from one segment to the next.
struct GradBufs { act_t *dx, *a, *b, *c, *d; };
// head: LayerNorm (f32) + average pool
static int head_bwd(const Exec& e, const float* d_out, const GradBufs& g) {
    const Model& m = *e.m; const Layout& L = *e.L; const GgTinyVitCfg& c = m.cfg;
    const int B = e.B, res = m.stages[2].res, T = res * res, C3 = c.embed_dims[3];
    const bool tr = e.tr(m.head.t_g);
    float* dpool = reinterpret_cast<float*>(g.a);
    if (c.features_only) GG_HIP(hipMemcpyAsync(dpool, d_out, (size_t)B * C3 * sizeof(float), hipMemcpyDeviceToDevice, e.st));
    else GG_TRY(gg_layernorm_bwd(d_out, e.F(L.pooled), 1, e.F(L.mean_h), e.F(L.rstd_h), e.P(m.head.t_g), B, C3, nullptr, dpool,
                                 e.F(L.lnscratch), tr ? e.Gd(m.head.t_g) : nullptr, tr ? e.Gd(m.head.t_b) : nullptr, 1, e.st));
    return token_mean_bwd(e, dpool, g.dx, B, T, C3);
}
// TinyVitBlock: x1 = x0 + s1*(proj(attn(qkv(ln1(x0))))+b); x2 = BN(dw(x1)); x3 = x2 + s2*(fc2(gelu(fc1(ln2(x2)))))
static int block_bwd(const Exec& e, int s, size_t i, int slot, const GradBufs& g) {
    const Model& m = *e.m; const Layout& L = *e.L; const Schedule& k = m.sch;
    const StageL& st = m.stages[s];
    const int B = e.B, C = st.C, hid = (int)(C * m.cfg.mlp_ratio), rps = st.res * st.res;
    const int64_t M = (int64_t)B * rps;
    const BlockL& l = st.blocks[i]; const BlockAct& a = L.blocks[s][i];
    const float *s1 = e.dropv(slot), *s2 = e.dropv(slot + 1);
    act_t *dx = g.dx, *t_a = g.a, *t_b = g.b, *t_c = g.c;
    if (block_compacts(e, s, i)) {
        // the frozen block over the kept samples' rows (block_compacts): the same launches as below, the branch tensors dh / db / do / dqkv / da compact
        GG_TRY(block_lists(e, slot));
        const int *l1 = e.drop_list(0), *l2 = e.drop_list(1);
        const RowMap in2 = {l2, rps, true, false}, cc2 = {l2, rps, false, false}, in1 = {l1, rps, true, false}, cc1 = {l1, rps, false, false};
        // dh = (s2*dx)[kept] . W2 * gelu'(hpre)  -> t_b;  db = dh . W1  -> t_a;  dx2 = LN2bwd(db) + dx (dropped samples: dx) + local_conv's column sums  -> t_b
        GG_TRY(gemm(e, dx, C, e.Wt(l.fc2), l.fc2.Np, t_b, hid, M, hid, C, nullptr, 0, nullptr, s2, rps, nullptr, nullptr, e.A(a.hpre), GG_ACT_GELU, &in2));
        GG_TRY(gemm(e, t_b, hid, e.Wt(l.fc1), l.fc1.Np, t_a, C, M, C, hid, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, &cc2));
        GG_TRY(gg_layernorm_bwd_map((const float*)t_a, (const float*)e.A(a.x2), e.F(a.mean2), e.F(a.rstd2), e.P(l.ln2.t_g), M, C, (const float*)dx, (float*)t_b,
                                    e.F(L.lnscratch), l2 + GG_DROP_LIST_HEAD + B, rps, e.st));
        GG_TRY(gg_bn_bwd_coef_from_x(e.F(L.lnscratch), gg_layernorm_bwd_colsum_rows(M), C, M, e.F(a.local.stat), e.P(l.local.bn.t_g), e.P(l.local.bn.t_b),
                                     bn_coef(e, M, C), e.st));
        GG_TRY(dw_bwd_data_fused(e, t_b, e.A(a.local.y), bn_coef(e, M, C), l.local.w, t_c, B, st.res, st.res, nullptr, nullptr, nullptr, nullptr, 0, nullptr));
        // do = (s1*dx1)[kept] . Wproj  -> t_a;  dqkv  -> t_b (the forward's qkv / out / lse at the physical window);  da = dqkv . Wqkv  -> t_a;  dx0 = LN1bwd(da) + dx1
        GG_TRY(gemm(e, t_c, C, e.Wt(l.proj), l.proj.Np, t_a, C, M, C, C, nullptr, 0, nullptr, s1, rps, nullptr, nullptr, nullptr, 0, &in1));
        GgAttnArgs at;
        attn_args(e, st, l, a, B, at);
        at.dout = t_a; at.lddo = C; at.dqkv = t_b;
        at.window_map = l1 + GG_DROP_LIST_HEAD; at.num_windows_dev = l1;
        GG_TRY(attention_run(e, at, true));      // (frozen block, single-pass kernel: no bias gradient, no dS region)
        GG_TRY(gemm(e, t_b, 3 * C, e.Wt(l.qkv), l.qkv.Np, t_a, C, M, C, 3 * C, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, &cc1));
        return gg_layernorm_bwd_map((const float*)t_a, (const float*)e.A(a.x0), e.F(a.mean1), e.F(a.rstd1), e.P(l.ln1.t_g), M, C, (const float*)t_c, (float*)dx, nullptr,
                                    l1 + GG_DROP_LIST_HEAD + B, rps, e.st);
    }
    // dx == d(x3).  MLP branch: dh = (s2*dx) . W2  * gelu'(hpre)      -> t_b  [M, hid]
    GG_TRY(gemm(e, dx, C, e.Wt(l.fc2), l.fc2.Np, t_b, hid, M, hid, C, nullptr, 0, nullptr, s2, rps, nullptr, nullptr, e.A(a.hpre), GG_ACT_GELU));
    if (e.tr(l.fc2.t_w)) {
        GG_TRY(dense_wgrad(e, l.fc2, e.A(a.h), hid, dx, C, M, s2, rps, false));
        GG_TRY(bias_grad(e, l.fc2.t_b, dx, C, M, C, s2, rps));
    }
    // db = dh . W1                                                     -> t_a  [M, C]
    GG_TRY(gemm(e, t_b, hid, e.Wt(l.fc1), l.fc1.Np, t_a, C, M, C, hid));
    if (e.tr(l.fc1.t_w)) {
        GG_TRY(dense_wgrad(e, l.fc1, e.A(a.b), C, t_b, hid, M, nullptr, 0, false));
        GG_TRY(bias_grad(e, l.fc1.t_b, t_b, hid, M, hid, nullptr, 0));
    }
    // dx2 = LN2bwd(db) + dx                                            -> t_b
    // frozen block: the same kernel also leaves (sum dx2*x2, sum dx2) per column, all that local_conv's BatchNorm backward needs
    const bool lncol = k.fuse_lncol && k.fuse_bnbwd && C <= 640 && !e.tr(l.local.w.t_w) && !e.tr(l.local.bn.t_g) && !e.tr(l.local.bn.t_b) &&
                       !e.tr(l.ln2.t_g) && !e.tr(l.ln2.t_b);       // (the fused form produces no LayerNorm / BatchNorm parameter gradients: every one of them must be frozen)
    if (lncol) {
        GG_TRY(gg_layernorm_bwd_colsum(t_a, e.A(a.x2), e.f32, e.F(a.mean2), e.F(a.rstd2), e.P(l.ln2.t_g), M, C, dx, t_b, e.F(L.lnscratch), e.st));
    } else {
        const bool tr = e.tr(l.ln2.t_g);
        GG_TRY(gg_layernorm_bwd(t_a, e.A(a.x2), e.f32, e.F(a.mean2), e.F(a.rstd2), e.P(l.ln2.t_g), M, C, dx, t_b, e.F(L.lnscratch),
                                tr ? e.Gd(l.ln2.t_g) : nullptr, tr ? e.Gd(l.ln2.t_b) : nullptr, 1, e.st));
    }
    // local_conv: x2 = BN(dw(x1)).  dy -> t_a (dz scratch t_c), dx1 = dwT(dy) -> t_c
    if (e.tr(l.local.w.t_w) || !k.fuse_bnbwd) {
        GG_TRY(bn_bwd(e, l.local.bn, a.local, M, GG_ACT_NONE, t_b, t_c, t_a));
        if (e.tr(l.local.w.t_w)) GG_TRY(dw_bwd_weight(e, l.local.w, e.A(a.x1), t_a, B, st.res, st.res, 1));
        GG_TRY(dw_bwd_data(e, l.local.w, t_a, t_c, B, st.res, st.res, 1));
    } else {
        // frozen taps: BN-backward apply is folded into the conv's staging (no dz / dy tensors at all)
        if (lncol) GG_TRY(gg_bn_bwd_coef_from_x(e.F(L.lnscratch), gg_layernorm_bwd_colsum_rows(M), C, M, e.F(a.local.stat), e.P(l.local.bn.t_g),
                                                e.P(l.local.bn.t_b), bn_coef(e, M, C), e.st));
        else GG_TRY(bn_bwd_reduce_fin(e, l.local.bn, a.local, M, GG_ACT_NONE, t_b, nullptr));
        GG_TRY(dw_bwd_data_fused(e, t_b, e.A(a.local.y), bn_coef(e, M, C), l.local.w, t_c, B, st.res, st.res, nullptr, nullptr, nullptr, nullptr, 0, nullptr));
    }
    act_t* dx1 = t_c;
    if (st.pres != st.res) {
        // padded block: the crop's adjoint is zero padding -- the branch runs at Mp rows on the padded map, the pad keys / values send their gradient into qkv's and
        // LayerNorm1's parameters (a pad query has dO = 0), and the gradient at the pad positions of the padded input is dropped by the crop
        const int rpsp = st.pres * st.pres;
        const int64_t Mp = (int64_t)B * rpsp;
        act_t* t_d = g.d;
        GG_TRY(window_pad(e, st, dx1, t_d));                                                               // dx1 on the padded map -> t_d  [Mp, C]
        GG_TRY(gemm(e, t_d, C, e.Wt(l.proj), l.proj.Np, t_a, C, Mp, C, C, nullptr, 0, nullptr, s1, rpsp));  // do -> t_a
        if (e.tr(l.proj.t_w)) {
            GG_TRY(dense_wgrad(e, l.proj, e.A(a.o), C, t_d, C, Mp, s1, rpsp, false));
            GG_TRY(bias_grad(e, l.proj.t_b, t_d, C, Mp, C, s1, rpsp));
        }
        GgAttnArgs at;
        attn_args(e, st, l, a, B, at);
        at.dout = t_a; at.lddo = C; at.dqkv = t_b;                                                         // dqkv -> t_b  [Mp, 3C]
        at.dbias = e.tr(l.t_ab) ? e.Gd(l.t_ab) : nullptr;
        GG_TRY(attention_bwd(e, st, at));
        GG_TRY(gemm(e, t_b, 3 * C, e.Wt(l.qkv), l.qkv.Np, t_a, C, Mp, C, 3 * C));                          // da -> t_a  [Mp, C]
        if (e.tr(l.qkv.t_w)) {
            GG_TRY(dense_wgrad(e, l.qkv, e.A(a.a), C, t_b, 3 * C, Mp, nullptr, 0, false));
            GG_TRY(bias_grad(e, l.qkv.t_b, t_b, 3 * C, Mp, 3 * C, nullptr, 0));
        }
        const act_t* xp = e.A(a.xpad);
        if (!xpad_kept(e, l)) { GG_TRY(window_pad(e, st, e.A(a.x0), t_d)); xp = t_d; }                     // (the forward's xpad was a temporary: formed again)
        const bool trp = e.tr(l.ln1.t_g);
        GG_TRY(gg_layernorm_bwd(t_a, xp, e.f32, e.F(a.mean1), e.F(a.rstd1), e.P(l.ln1.t_g), Mp, C, nullptr, t_b, e.F(L.lnscratch),
                                trp ? e.Gd(l.ln1.t_g) : nullptr, trp ? e.Gd(l.ln1.t_b) : nullptr, 1, e.st));  // d(xpad) -> t_b  [Mp, C]
        return window_crop_add(e, st, t_b, dx1, nullptr, dx);                                              // dx0 = dx1 + crop(d(xpad))
    }
    // attention branch: do = (s1*dx1) . Wproj                          -> t_a  [M, C]
    GG_TRY(gemm(e, dx1, C, e.Wt(l.proj), l.proj.Np, t_a, C, M, C, C, nullptr, 0, nullptr, s1, rps));
    if (e.tr(l.proj.t_w)) {
        GG_TRY(dense_wgrad(e, l.proj, e.A(a.o), C, dx1, C, M, s1, rps, false));
        GG_TRY(bias_grad(e, l.proj.t_b, dx1, C, M, C, s1, rps));
    }
    // dqkv                                                             -> t_b  [M, 3C]
    GgAttnArgs at;
    attn_args(e, st, l, a, B, at);
    at.dout = t_a; at.lddo = C; at.dqkv = t_b;
    at.dbias = e.tr(l.t_ab) ? e.Gd(l.t_ab) : nullptr;
    GG_TRY(attention_bwd(e, st, at));
    // da = dqkv . Wqkv                                                 -> t_a  [M, C]
    GG_TRY(gemm(e, t_b, 3 * C, e.Wt(l.qkv), l.qkv.Np, t_a, C, M, C, 3 * C));
    if (e.tr(l.qkv.t_w)) {
        GG_TRY(dense_wgrad(e, l.qkv, e.A(a.a), C, t_b, 3 * C, M, nullptr, 0, false));
        GG_TRY(bias_grad(e, l.qkv.t_b, t_b, 3 * C, M, 3 * C, nullptr, 0));
    }
    // dx0 = LN1bwd(da) + dx1                                           -> dx (the block-output gradient is dead by now)
    const bool tr = e.tr(l.ln1.t_g);
    return gg_layernorm_bwd(t_a, e.A(a.x0), e.f32, e.F(a.mean1), e.F(a.rstd1), e.P(l.ln1.t_g), M, C, dx1, dx, e.F(L.lnscratch),
                            tr ? e.Gd(l.ln1.t_g) : nullptr, tr ? e.Gd(l.ln1.t_b) : nullptr, 1, e.st);
}
// PatchMerging: out = BN3(conv3(a2)); a2 = gelu(BN2(dw s2(a1))); a1 = gelu(BN1(conv1(x)))
static int merge_bwd(const Exec& e, int s, const GradBufs& g) {
    const Model& m = *e.m; const Layout& L = *e.L; const Schedule& k = m.sch;
    const StageL& st = m.stages[s];
    const ConvBNDense& c1 = st.merge.c1; const ConvBNDw& c2 = st.merge.c2; const ConvBNDense& c3 = st.merge.c3;
    const MergeAct& ma = L.merge[s];
    const int B = e.B, C = st.C, rin = s == 0 ? m.res0 : m.stages[s - 1].res, Cin = s == 0 ? m.cfg.embed_dims[0] : m.stages[s - 1].C;
    const int64_t M = (int64_t)B * st.res * st.res, Min = (int64_t)B * rin * rin;
    act_t *dx = g.dx, *t_a = g.a, *t_b = g.b, *t_c = g.c, *t_d = g.d;
    GG_TRY(bn_bwd(e, c3.bn, ma.c3, M, GG_ACT_NONE, dx, t_b, t_a));                                     // dy3 -> t_a
    if (e.tr(c3.w.t_w)) GG_TRY(dense_wgrad(e, c3.w, e.A(ma.a2), C, t_a, C, M, nullptr, 0, false));
    if (k.fuse_bngemm && !e.tr(c1.w.t_w) && !e.tr(c2.w.t_w) && C % 64 == 0) {
        // frozen chain: BatchNorm2's reduce rides on conv3's dgrad, BatchNorm1's apply is folded into conv1's
        GG_TRY(gemm_bnbwd(e, t_a, C, e.Wt(c3.w), c3.w.Np, t_d, M, C, C, c2.bn, ma.c2, GG_ACT_GELU));   // dz2 -> t_d
        act_t* dz1;
        if (k.fuse_bnbwd && k.fuse_bnbwd_epi) {
            // the stride-2 data gradient forms dy2 from (dz2, y2) at its taps and emits dz1 = da1*GELU'(BN1(y1)) + BN1's sums
            GG_TRY(dw_bwd_data_fused_fin(e, c2.w, t_d, e.A(ma.c2.y), bn_coef(e, M, C), t_b, B, rin, rin, 2, c1.bn, ma.c1));   // dz1 -> t_b
            dz1 = t_b;
        } else {
            GG_TRY(bn_bwd_apply_only(e, t_d, e.A(ma.c2.y), bn_coef(e, M, C), M, C, t_a));              // dy2 -> t_a
            GG_TRY(dw_bwd_data(e, c2.w, t_a, t_b, B, rin, rin, 2));                                    // da1 -> t_b [Min, C]
            GG_TRY(bn_bwd_reduce_fin(e, c1.bn, ma.c1, Min, GG_ACT_GELU, t_b, t_d));                    // dz1 -> t_d
            dz1 = t_d;
        }
        return gemm_folded_dgrad(e, c1.w, dz1, e.A(ma.c1.y), bn_coef(e, Min, C), e.F(ma.c1.stat), dx, Min, nullptr);
    }
    GG_TRY(gemm(e, t_a, C, e.Wt(c3.w), c3.w.Np, t_b, C, M, C, C));                                     // da2 -> t_b
    GG_TRY(bn_bwd(e, c2.bn, ma.c2, M, GG_ACT_GELU, t_b, t_c, t_a));                                    // dy2 -> t_a
    if (e.tr(c2.w.t_w)) GG_TRY(dw_bwd_weight_act1(e, c2.w, c1.bn, ma.c1, ma.a1, t_a, B, rin, rin, 2));
    GG_TRY(dw_bwd_data(e, c2.w, t_a, t_b, B, rin, rin, 2));                                            // da1 -> t_b [Min, C]
    GG_TRY(bn_bwd(e, c1.bn, ma.c1, Min, GG_ACT_GELU, t_b, t_c, t_a));                                  // dy1 -> t_a
    if (e.tr(c1.w.t_w)) GG_TRY(dense_wgrad(e, c1.w, e.A(merge_input(L, s)), Cin, t_a, C, Min, nullptr, 0, false));
    return gemm(e, t_a, C, e.Wt(c1.w), c1.w.Np, dx, Cin, Min, Cin, C);                                 // dx_in -> dx
}
// MBConv: out = gelu(x + s*BN3(conv3(a2))); a2 = gelu(BN2(dw(a1))); a1 = gelu(BN1(conv1(x)))
static int mbconv_bwd(const Exec& e, size_t i, int slot, const GradBufs& g) {
    const Model& m = *e.m; const Layout& L = *e.L; const Schedule& k = m.sch;
    const int B = e.B, H0 = m.res0, C0 = m.cfg.embed_dims[0];
    const int64_t M0 = (int64_t)B * H0 * H0;
    const int mid = (int)(C0 * m.cfg.mbconv_expand_ratio);
    const MBConvL& l = m.mb[i]; const MBAct& a = L.mb[i];
    act_t *dx = g.dx, *t_a = g.a, *t_b = g.b, *t_c = g.c, *t_d = g.d;
    // dz(=dpre, also the skip gradient) -> t_b, dy3 -> t_a
    GG_TRY(bn_bwd(e, l.c3.bn, a.c3, M0, GG_ACT_GELU, dx, t_b, t_a, e.A(a.x), e.dropv(slot), H0 * H0));
    // (a2 exists: the forward only skips it when its `trainable` mask freezes conv3 -- the two calls must get the same mask)
    if (e.tr(l.c3.w.t_w)) GG_TRY(dense_wgrad(e, l.c3.w, e.A(a.a2), mid, t_a, C0, M0, nullptr, 0, false));
    const bool reduce_on_dgrad = k.fuse_bngemm && mid % 64 == 0;      // BatchNorm2's reduce rides in the epilogue of conv3's dgrad
    const bool reduce_on_dw = k.fuse_bnbwd && k.fuse_bnbwd_epi;       // BatchNorm1's reduce rides in the epilogue of the depthwise data gradient
    if (reduce_on_dgrad && !e.tr(l.c1.w.t_w) && !e.tr(l.c2.w.t_w)) {
        // frozen chain: no dy tensor at all -- BatchNorm1's apply is folded into conv1's dgrad
        GG_TRY(gemm_bnbwd(e, t_a, C0, e.Wt(l.c3.w), l.c3.w.Np, t_d, M0, mid, C0, l.c2.bn, a.c2, GG_ACT_GELU));             // dz2 -> t_d
        act_t* dz1;
        if (reduce_on_dw) {
            GG_TRY(dw_bwd_data_fused_fin(e, l.c2.w, t_d, e.A(a.c2.y), bn_coef(e, M0, mid), t_c, B, H0, H0, 1, l.c1.bn, a.c1));   // dz1 -> t_c
            dz1 = t_c;
        } else {
            if (k.fuse_bnbwd) {      // dy2 is formed from (dz2, y2) inside the conv; da1 -> t_c
                GG_TRY(dw_bwd_data_fused(e, t_d, e.A(a.c2.y), bn_coef(e, M0, mid), l.c2.w, t_c, B, H0, H0, nullptr, nullptr, nullptr, nullptr, 0, nullptr));
            } else {
                GG_TRY(bn_bwd_apply_only(e, t_d, e.A(a.c2.y), bn_coef(e, M0, mid), M0, mid, t_a));                         // dy2 -> t_a
                GG_TRY(dw_bwd_data(e, l.c2.w, t_a, t_c, B, H0, H0, 1));                                                    // da1 -> t_c
            }
            GG_TRY(bn_bwd_reduce_fin(e, l.c1.bn, a.c1, M0, GG_ACT_GELU, t_c, t_d));                                        // dz1 -> t_d
            dz1 = t_d;
        }
        return gemm_folded_dgrad(e, l.c1.w, dz1, e.A(a.c1.y), bn_coef(e, M0, mid), e.F(a.c1.stat), dx, M0, t_b);           // + dpre
    }
    // dy1 in t_a: conv1's weight gradient, then dx_in = dy1 . W1 + dpre -> dx
    auto conv1_bwd = [&]() -> int {
        if (e.tr(l.c1.w.t_w)) GG_TRY(dense_wgrad(e, l.c1.w, e.A(a.x), C0, t_a, mid, M0, nullptr, 0, false));
        return gemm(e, t_a, mid, e.Wt(l.c1.w), l.c1.w.Np, dx, C0, M0, C0, mid, nullptr, 0, nullptr, nullptr, 0, t_b);
    };
    if (reduce_on_dgrad && reduce_on_dw) {
        // trainable weights: dy2 / dy1 are materialised for the weight gradients, but both BatchNorm-backward REDUCE passes still
        // ride on the kernels that produce their inputs (conv3's dgrad epilogue, the depthwise data gradient's epilogue)
        GG_TRY(gemm_bnbwd(e, t_a, C0, e.Wt(l.c3.w), l.c3.w.Np, t_d, M0, mid, C0, l.c2.bn, a.c2, GG_ACT_GELU));             // dz2 -> t_d
        GG_TRY(bn_bwd_apply_only(e, t_d, e.A(a.c2.y), bn_coef(e, M0, mid), M0, mid, t_a));                                 // dy2 -> t_a
        if (e.tr(l.c2.w.t_w)) GG_TRY(dw_bwd_weight_act1(e, l.c2.w, l.c1.bn, a.c1, a.a1, t_a, B, H0, H0, 1));
        GG_TRY(dw_bwd_data_fused_fin(e, l.c2.w, t_a, nullptr, nullptr, t_c, B, H0, H0, 1, l.c1.bn, a.c1));                 // dz1 -> t_c
        GG_TRY(bn_bwd_apply_only(e, t_c, e.A(a.c1.y), bn_coef(e, M0, mid), M0, mid, t_a));                                 // dy1 -> t_a
        return conv1_bwd();
    }
    GG_TRY(gemm(e, t_a, C0, e.Wt(l.c3.w), l.c3.w.Np, t_c, mid, M0, mid, C0));                                              // da2 -> t_c [M0, mid]
    if (e.tr(l.c2.w.t_w) || !reduce_on_dw) {
        GG_TRY(bn_bwd(e, l.c2.bn, a.c2, M0, GG_ACT_GELU, t_c, t_d, t_a));                                                  // dy2 -> t_a
        if (e.tr(l.c2.w.t_w)) GG_TRY(dw_bwd_weight_act1(e, l.c2.w, l.c1.bn, a.c1, a.a1, t_a, B, H0, H0, 1));
        GG_TRY(dw_bwd_data(e, l.c2.w, t_a, t_c, B, H0, H0, 1));                                                            // da1 -> t_c
        GG_TRY(bn_bwd(e, l.c1.bn, a.c1, M0, GG_ACT_GELU, t_c, t_d, t_a));                                                  // dy1 -> t_a
    } else {
        // frozen taps: 3 streaming passes instead of 5.  reduce(c2) -> dz2; the depthwise data gradient forms dy2 from
        // (dz2, y2) while staging and emits dz1 = da1*GELU'(BN1(y1)) + BN1's backward statistics; apply(c1) -> dy1.
        GG_TRY(bn_bwd_reduce_fin(e, l.c2.bn, a.c2, M0, GG_ACT_GELU, t_c, t_d));                                            // dz2 -> t_d
        GG_TRY(dw_bwd_data_fused_fin(e, l.c2.w, t_d, e.A(a.c2.y), bn_coef(e, M0, mid), t_c, B, H0, H0, 1, l.c1.bn, a.c1)); // dz1 -> t_c
        GG_TRY(bn_bwd_apply_only(e, t_c, e.A(a.c1.y), bn_coef(e, M0, mid), M0, mid, t_a));                                 // dy1 -> t_a
    }
    return conv1_bwd();
}
// PatchEmbed (dgrad only to conv1's output; the image needs no gradient)
static int patch_embed_bwd(const Exec& e, const GradBufs& g) {
    const Model& m = *e.m; const Layout& L = *e.L;
    const int B = e.B, H1 = m.cfg.img_size / 2, H0 = m.res0, C0 = m.cfg.embed_dims[0];
    const int64_t M1 = (int64_t)B * H1 * H1, M0 = (int64_t)B * H0 * H0;
    act_t *dx = g.dx, *t_a = g.a, *t_b = g.b, *t_c = g.c, *t_d = g.d;
    const bool need1 = e.tr(m.pe1.w.t_w) || e.tr(m.pe1.bn.t_g);
    const bool need2 = e.tr(m.pe2.w.t_w) || e.tr(m.pe2.bn.t_g) || need1;
    // (conv2 keeps the three-pass BatchNorm backward: forming dy2 from (dx, y2) inside both of its GEMMs was measured at +1.7 ms of GEMM time
    // against the 0.75 ms apply pass it removes -- the two-source prologue kernel at K = 96 runs at 62 TFLOP/s, the plain one at 86)
    if (need2) {
        GG_TRY(bn_bwd(e, m.pe2.bn, L.pe2, M0, GG_ACT_NONE, dx, t_b, t_a));                             // dy2 -> t_a [M0, C0]
        if (e.tr(m.pe2.w.t_w)) GG_TRY(dense_wgrad(e, m.pe2.w, e.A(L.col2), m.pe2.w.Kp, t_a, C0, M0, nullptr, 0, true));
    }
    if (!need1) return 0;
    const bool fuse1 = m.sch.fuse_bnbwd && m.pe1.w.N == m.pe1.bn.C && (m.pe1.bn.C & (e.f32 ? 3 : 7)) == 0;
    // fp32_split: conv2's data gradient by input parity with BN1's backward reduce as epilogue -- no dcol2 (5.5 GB at 1024 images, written once and read once).  Taken
    // exactly where the dcol2 product below would run as a split product (so the split launch count of a step does not depend on the route) and the shape qualifies:
    // an even map, 48 input channels, Cout % 32 == 0.  Everything else keeps the two launches.  (The backward alone decides: the forward saves nothing for either route.)
    const bool parity = fuse1 && m.split && e.f32 && !gg_dev_env("GG_NO_PE2_DGRAD_PARITY") && m.pe2.w.Np == C0 &&
                        ((M0 + 127) / 128) * ((m.pe2.w.Kp + 127) / 128) >= split_min_tiles() && planes_of(e, e.Wt(m.pe2.w), m.pe2.w.Np, m.pe2.w.Kp) != nullptr &&
                        gg_conv3x3s2_dgrad_fits(H1, H1, C0 / 2, C0) != 0 && gg_conv3x3s2_dgrad_planes_bytes(C0 / 2, C0) <= M0 * m.pe2.w.Kp * (int64_t)sizeof(float);
    if (parity) return convnorm_wgrad_from_dz(e, m.pe1, L.pe1, M1, GG_ACT_GELU, t_d, e.A(L.col1), 32, t_b, B, H1, H1, &m.pe2, t_a);      // (t_b: the weight's plane scratch)
    GG_TRY(gemm(e, t_a, C0, e.Wt(m.pe2.w), m.pe2.w.Np, t_b, m.pe2.w.Kp, M0, m.pe2.w.Kp, C0));          // dcol2 -> t_b
    if (fuse1) {
        // col2im + BN1-backward reduce in one pass (dz1 -> t_d; da1 and dy1 are never formed), weight gradient from (dz1, y1, coef)
        return convnorm_wgrad_from_dz(e, m.pe1, L.pe1, M1, GG_ACT_GELU, t_d, e.A(L.col1), 32, t_b, B, H1, H1);
    }
    GG_TRY(col2im(e, t_b, t_c, B, H1, H1, C0 / 2));                                                    // da1 -> t_c [M1, C0/2]
    GG_TRY(bn_bwd(e, m.pe1.bn, L.pe1, M1, GG_ACT_GELU, t_c, t_d, t_a));                                // dy1 -> t_a
    if (e.tr(m.pe1.w.t_w)) GG_TRY(dense_wgrad(e, m.pe1.w, e.A(L.col1), 32, t_a, C0 / 2, M1, nullptr, 0, true));
    return 0;
}
static int segment_bwd(const Exec& e, const Segment& sg, const GradBufs& g) {
    if (sg.kind == SEG_MBCONV) return mbconv_bwd(e, (size_t)sg.index, sg.slot, g);
    return sg.kind == SEG_MERGE ? merge_bwd(e, sg.stage - 1, g) : block_bwd(e, sg.stage - 1, (size_t)sg.index, sg.slot, g);
}
// The driver: the forward's segments from the end, each replayed first under activation recompute (its tensors are re-formed in the segment
// region right before its backward).  done(S): every launch of model stage S is enqueued, its parameter gradients are final (-1: all of them).
static int backward_impl(const Exec& e, const float* d_out) {
    const Model& m = *e.m; const Layout& L = *e.L;
    const GradBufs g = {e.A(L.G[0]), e.A(L.G[1]), e.A(L.G[2]), e.A(L.G[3]), e.A(L.G[4])};
    Exec r = e;          // the replaying executor takes e's routes: same flags, same mask, training
    r.replay = true;
    GG_TRY(head_bwd(e, d_out, g));
    int stage = 3;
    for (auto sg = m.segs.rbegin(); sg != m.segs.rend(); ++sg) {
        for (; stage > sg->stage; --stage) e.done(stage);
        if (m.cfg.recompute) GG_TRY(segment_fwd(r, *sg));
        GG_TRY(segment_bwd(e, *sg, g));
    }
    for (; stage >= 0; --stage) e.done(stage);
    GG_TRY(patch_embed_bwd(e, g));
    e.done(-1);
    return 0;
}

// Wn [N][ldn] and Wt [ldn][ldt] (ldn = K rounded up to 8, ldt = N rounded up to 8): the padding columns / rows of both copies are written as zeros
// here, so the cache needs no zero-initialisation by its owner (the GEMMs contract over ldn, the split-plane copies are taken over the padded shapes)
template <typename T>
__global__ void repack_weight_kernel(const float* __restrict__ src, int N, int cin, int taps, T* __restrict__ Wn, int ldn,
                                     T* __restrict__ Wt, int ldt) {
    const int K = cin * taps;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ldt * ldn) return;
    const int co = i / ldn, k = i % ldn;
    T v = (T)0.f;
    if (co < N && k < K) {
        const int tap = k / cin, ci = k % cin;
        v = (T)src[((int64_t)co * cin + ci) * taps + tap];
    }
    if (co < N) Wn[(int64_t)co * ldn + k] = v;
    Wt[(int64_t)k * ldt + co] = v;
}
__global__ void repack_taps_kernel(const float* __restrict__ src, int C, float* __restrict__ taps) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 9 * C) return;
    const int t = i / C, c = i % C;
    taps[i] = src[c * 9 + t];
}
static int repack_dense(const DenseW& w, const float* params, const Model& m, char* wc, hipStream_t st) {
    const int n = w.Np * w.Kp;        // padded: the kernel zeroes the padding of both copies
    if (m.f32)
        hipLaunchKernelGGL(repack_weight_kernel<float>, dim3((unsigned)gg_cdiv(n, 256)), dim3(256), 0, st, params + m.tensors[w.t_w].offset, w.N,
                           w.cin, w.taps, reinterpret_cast<float*>(wc + w.wn), w.Kp, reinterpret_cast<float*>(wc + w.wt), w.Np);
    else
        hipLaunchKernelGGL(repack_weight_kernel<bf16>, dim3((unsigned)gg_cdiv(n, 256)), dim3(256), 0, st, params + m.tensors[w.t_w].offset, w.N,
                           w.cin, w.taps, reinterpret_cast<bf16*>(wc + w.wn), w.Kp, reinterpret_cast<bf16*>(wc + w.wt), w.Np);
    GG_LAUNCH_CHECK();
    return 0;
}
static int repack_dw(const DwW& w, const float* params, const Model& m, char* wc, hipStream_t st) {
    hipLaunchKernelGGL(repack_taps_kernel, dim3((unsigned)gg_cdiv(9 * w.C, 256)), dim3(256), 0, st, params + m.tensors[w.t_w].offset, w.C,
                       reinterpret_cast<float*>(wc + w.taps));
    GG_LAUNCH_CHECK();
    return 0;
}

}  // namespace

// ------------------------------------------------------------------------------------------- C ABI
extern "C" int gg_tinyvit_num_tensors(const GgTinyVitCfg* cfg) {
    Model m;
    if (build_model(cfg, m)) return -1;
    return (int)m.tensors.size();
}
extern "C" int gg_tinyvit_tensor_info(const GgTinyVitCfg* cfg, int i, char* name, int name_cap, int64_t* offset, int64_t* numel,
                                      int* ndim, int64_t* shape4, int* kind) {
    Model m;
    GG_TRY(build_model(cfg, m));
    GG_CHECK(i >= 0 && i < (int)m.tensors.size(), "gg_tinyvit_tensor_info: index %d out of range", i);
    const TensorInfo& t = m.tensors[i];
    if (name && name_cap > 0) snprintf(name, name_cap, "%s", t.name.c_str());
    if (offset) *offset = t.offset;
    if (numel) *numel = t.numel;
    if (ndim) *ndim = t.ndim;
    if (shape4) for (int j = 0; j < 4; ++j) shape4[j] = t.shape[j];
    if (kind) *kind = t.kind;
    return 0;
}
extern "C" int64_t gg_tinyvit_param_floats(const GgTinyVitCfg* cfg) { Model m; return build_model(cfg, m) ? -1 : m.param_floats; }
extern "C" int64_t gg_tinyvit_buffer_floats(const GgTinyVitCfg* cfg) { Model m; return build_model(cfg, m) ? -1 : m.buffer_floats; }
extern "C" int gg_tinyvit_num_counters(const GgTinyVitCfg* cfg) { Model m; return build_model(cfg, m) ? -1 : m.num_counters; }
extern "C" int gg_tinyvit_num_drop_slots(const GgTinyVitCfg* cfg) { Model m; return build_model(cfg, m) ? -1 : m.drop_slots; }
extern "C" int64_t gg_tinyvit_wcache_bytes(const GgTinyVitCfg* cfg) { Model m; return build_model(cfg, m) ? -1 : m.wcache_bytes; }
extern "C" int64_t gg_tinyvit_workspace_bytes_masked(const GgTinyVitCfg* cfg, int batch, int training, const uint8_t* trainable) {
    Model m;
    if (build_model(cfg, m)) return -1;
    if (batch <= 0) { gg_set_error("gg_tinyvit_workspace_bytes: batch must be > 0"); return -1; }
    Plan p; Layout L;
    plan_make(m, batch, training != 0, p, L, trainable);
    return p.total;
}
extern "C" int64_t gg_tinyvit_workspace_bytes(const GgTinyVitCfg* cfg, int batch, int training) {
    return gg_tinyvit_workspace_bytes_masked(cfg, batch, training, nullptr);
}
extern "C" int gg_tinyvit_activation_info_masked(const GgTinyVitCfg* cfg, int batch, const char* name, const uint8_t* trainable, int64_t* offset,
                                                 int64_t* bytes) {
    Model m;
    GG_TRY(build_model(cfg, m));
    Plan p; Layout L;
    plan_make(m, batch, true, p, L, trainable);
    auto it = p.index.find(name);
    GG_CHECK(it != p.index.end(), "gg_tinyvit_activation_info: no activation named '%s'", name);
    GG_CHECK(!p.recomputed.count(name), "gg_tinyvit_activation_info: '%s' is not retained with activation recompute (recompute = 1: a segment-internal tensor that the backward recomputes in the shared segment region)", name);
    GG_CHECK(!p.temps.count(name), "gg_tinyvit_activation_info: '%s' is not retained under this trainable mask (a temporary between its producer and its one consumer)", name);
    if (offset) *offset = p.regs[it->second].offset;
    if (bytes) *bytes = p.regs[it->second].bytes;
    return 0;
}
extern "C" int gg_tinyvit_activation_info(const GgTinyVitCfg* cfg, int batch, const char* name, int64_t* offset, int64_t* bytes) {
    return gg_tinyvit_activation_info_masked(cfg, batch, name, nullptr, offset, bytes);
}
// include/gg_cls.h: where the inference forward leaves the last TinyVitBlock's output (timm forward_features).  Nothing after that block takes a slot of
// the inference ring (head.* and the scratch regions are persistent), so the map survives until the next forward on this workspace.
extern "C" int gg_tinyvit_last_map_info(const GgTinyVitCfg* cfg, int batch, int64_t* offset, int64_t* bytes, int* res, int* channels) {
    Model m;
    GG_TRY(build_model(cfg, m));
    GG_CHECK(batch > 0, "gg_tinyvit_last_map_info: batch must be > 0");
    Plan p; Layout L;
    plan_make(m, batch, false, p, L, nullptr);
    const std::string name = "stages.3.blocks." + std::to_string(m.stages[2].blocks.size() - 1) + ".out";
    auto it = p.index.find(name);
    GG_CHECK(it != p.index.end(), "gg_tinyvit_last_map_info: no activation named '%s'", name.c_str());
    if (offset) *offset = p.regs[it->second].offset;
    if (bytes) *bytes = (int64_t)batch * m.stages[2].res * m.stages[2].res * m.stages[2].C * m.es;
    if (res) *res = m.stages[2].res;
    if (channels) *channels = m.stages[2].C;
    return 0;
}
// `only` (host, one byte per tensor, or NULL = every tensor): the tensors whose cached forms are rebuilt.  After an optimizer step only the
// trainable tensors changed -- under the reference freeze policy 14 of the 52 cached matrices -- so the per-step refresh skips the frozen ones.
static int refresh_weights(const GgTinyVitCfg* cfg, const float* params, void* wcache, const uint8_t* only, void* stream);
extern "C" int gg_tinyvit_refresh_weights(const GgTinyVitCfg* cfg, const float* params, void* wcache, void* stream) {
    return refresh_weights(cfg, params, wcache, nullptr, stream);
}
extern "C" int gg_tinyvit_refresh_weights_masked(const GgTinyVitCfg* cfg, const float* params, void* wcache, const uint8_t* only, void* stream) {
    return refresh_weights(cfg, params, wcache, only, stream);
}
static int refresh_weights(const GgTinyVitCfg* cfg, const float* params, void* wcache, const uint8_t* only, void* stream) {
    Model m;
    GG_TRY(build_model(cfg, m));
    GG_CHECK(params && wcache, "gg_tinyvit_refresh_weights: null pointer");
    char* wc = (char*)wcache;
    hipStream_t st = (hipStream_t)stream;
    auto repack_dense = [&](const DenseW& w, const float* pp, const Model& mm, char* c, hipStream_t s) -> int {
        if (only && !only[w.t_w]) return 0;
        GG_TRY(::repack_dense(w, pp, mm, c, s));
        if (w.wn3 >= 0) GG_TRY(gg_split3_bf16(reinterpret_cast<const float*>(c + w.wn), w.N, w.Kp, w.Kp, c + w.wn3, s));
        if (w.wt3 >= 0) GG_TRY(gg_split3_bf16(reinterpret_cast<const float*>(c + w.wt), w.Kp, w.Np, w.Np, c + w.wt3, s));
        return 0;
    };
    auto repack_dw = [&](const DwW& w, const float* pp, const Model& mm, char* c, hipStream_t s) -> int {
        return (only && !only[w.t_w]) ? 0 : ::repack_dw(w, pp, mm, c, s);
    };
    GG_TRY(repack_dense(m.pe1.w, params, m, wc, st));
    GG_TRY(repack_dense(m.pe2.w, params, m, wc, st));
    for (auto& l : m.mb) {
        GG_TRY(repack_dense(l.c1.w, params, m, wc, st));
        GG_TRY(repack_dw(l.c2.w, params, m, wc, st));
        GG_TRY(repack_dense(l.c3.w, params, m, wc, st));
    }
    for (int s = 0; s < 3; ++s) {
        GG_TRY(repack_dense(m.stages[s].merge.c1.w, params, m, wc, st));
        GG_TRY(repack_dw(m.stages[s].merge.c2.w, params, m, wc, st));
        GG_TRY(repack_dense(m.stages[s].merge.c3.w, params, m, wc, st));
        for (auto& b : m.stages[s].blocks) {
            GG_TRY(repack_dense(b.qkv, params, m, wc, st));
            GG_TRY(repack_dense(b.proj, params, m, wc, st));
            GG_TRY(repack_dense(b.fc1, params, m, wc, st));
            GG_TRY(repack_dense(b.fc2, params, m, wc, st));
            GG_TRY(repack_dw(b.local.w, params, m, wc, st));
            if (b.bias_full >= 0 && !(only && !only[b.t_ab]))
                GG_TRY(gg_attention_expand_bias(params + m.tensors[b.t_ab].offset, m.stages[s].heads, m.stages[s].ws, kAttnScale,
                                                wc + b.bias_full, stream));
        }
    }
    return 0;
}
extern "C" int gg_tinyvit_set_drop_compact(int on) { return g_drop_compact.exchange(on != 0 ? 1 : 0); }
extern "C" int gg_tinyvit_set_attention16(int on) { return g_attention16.exchange(on != 0 ? 1 : 0); }
extern "C" int gg_tinyvit_set_attention16_train(int on) { return g_attention16_train.exchange(on != 0 ? 1 : 0); }
extern "C" int gg_tinyvit_set_deterministic_dbias(int on) { return g_deterministic_dbias.exchange(on != 0 ? 1 : 0); }
extern "C" int gg_tinyvit_forward(const GgTinyVitCfg* cfg, int batch, int training, const float* params, float* buffers,
                                  int64_t* counters, const void* wcache, const float* x, const float* drop_scales, void* workspace,
                                  float* out, const uint8_t* trainable, void* stream) {
    Model m;
    GG_TRY(build_model(cfg, m));
    GG_CHECK(batch > 0 && params && buffers && wcache && x && workspace && out, "gg_tinyvit_forward: null pointer / bad batch");
    GG_CHECK(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)wcache & 255) == 0, "gg_tinyvit_forward: workspace/wcache must be 256-byte aligned");
    Plan p; Layout L;
    plan_make(m, batch, training != 0, p, L, trainable);
    const bool compact = g_drop_compact.load() != 0;
    const bool attn16 = training == 0 && !m.f32 && g_attention16.load() != 0;      // (m.f32 covers fp32 and fp32_split)
    const bool attn16_train = training != 0 && !m.f32 && g_attention16_train.load() != 0;
    auto body = [&](hipStream_t st) -> int {
        Exec e(m, L, batch, training != 0);
        e.params = params; e.buffers = buffers; e.counters = counters;
        e.wc = (const char*)wcache; e.ws = (char*)workspace; e.st = st; e.drop = drop_scales; e.grads = nullptr;
        e.trainable = trainable;       // NULL: keep every activation a weight gradient could need
        e.compact = compact;
        e.attn16 = attn16;
        e.attn16_train = attn16_train;
        return forward_impl(e, x, out);
    };
    // launch-bound sizes (a serving panorama, small training batches: a few hundred launches of microseconds each) replay a captured graph
    if (!gg_graph_wanted((int64_t)batch * cfg->img_size * cfg->img_size <= (int64_t)64 * 224 * 224)) return body((hipStream_t)stream);
    GgGraphKey key;
    key.add('F').add_bytes(cfg, sizeof(*cfg)).add(batch).add(training).add(params).add(buffers).add(counters).add(wcache).add(x).add(drop_scales).add(workspace).add(out).add((int)compact)
       .add((int)attn16).add((int)attn16_train).add_bytes(trainable, trainable ? m.tensors.size() : 0);
    return gg_graph_run(key, (hipStream_t)stream, body);
}
extern "C" int gg_tinyvit_backward(const GgTinyVitCfg* cfg, int batch, const float* params, const void* wcache, const float* drop_scales,
                                   void* workspace, const float* d_out, float* grads, const uint8_t* trainable, void* stream,
                                   GgStageDoneFn stage_done, void* stage_user) {
    Model m;
    GG_TRY(build_model(cfg, m));
    GG_CHECK(batch > 0 && params && wcache && workspace && d_out && grads, "gg_tinyvit_backward: null pointer / bad batch");
    Plan p; Layout L;
    plan_make(m, batch, true, p, L, trainable);          // the SAME mask the training forward was called with: it decides the workspace layout
    Exec e(m, L, batch, true);
    e.params = params; e.buffers = nullptr; e.counters = nullptr;
    e.wc = (const char*)wcache; e.ws = (char*)workspace; e.st = (hipStream_t)stream; e.drop = drop_scales; e.grads = grads;
    e.trainable = trainable; e.stage_done = stage_done; e.stage_user = stage_user;
    e.compact = g_drop_compact.load() != 0;
    e.attn16_train = !m.f32 && g_attention16_train.load() != 0;      // the attention backward and the recompute replay (a training forward)
    e.det_dbias = g_deterministic_dbias.load() != 0;
    if (trainable) {
        // The schedule forms the two gradients of a (weight, bias) / (gamma, beta) pair together (BatchNorm / LayerNorm finalize kernels, the fused
        // frozen-chain forms): a mask that trains one tensor of a pair and freezes the other has no schedule -- refuse it by name instead of silently
        // leaving a gradient at zero.  (Every policy of the reference freezes whole modules: models/tinyvit.py:90-111.)
        std::map<std::string, int> by_name;
        for (size_t i = 0; i < m.tensors.size(); ++i) if (m.tensors[i].kind == GG_KIND_PARAM) by_name[m.tensors[i].name] = (int)i;
        for (const auto& kv : by_name) {
            const std::string& n = kv.first;
            if (n.size() < 7 || n.compare(n.size() - 7, 7, ".weight") != 0) continue;
            const auto it = by_name.find(n.substr(0, n.size() - 7) + ".bias");
            if (it == by_name.end()) continue;
            GG_CHECK((trainable[kv.second] != 0) == (trainable[it->second] != 0),
                     "gg_tinyvit_backward: %s and %s must be trainable or frozen together (requires_grad differs within the pair)", n.c_str(), it->first.c_str());
        }
    }
    if (stage_done || !gg_graph_wanted((int64_t)batch * cfg->img_size * cfg->img_size <= (int64_t)64 * 224 * 224))      // a host callback per stage (N > 1): eager
        return backward_impl(e, d_out);
    auto body = [&](hipStream_t st) -> int {
        Exec g = e;
        g.st = st;
        return backward_impl(g, d_out);
    };
    GgGraphKey key;
    key.add('B').add_bytes(cfg, sizeof(*cfg)).add(batch).add(params).add(wcache).add(drop_scales).add(workspace).add(d_out).add(grads).add((int)e.compact).add((int)e.attn16_train).add((int)e.det_dbias)
       .add_bytes(trainable, trainable ? m.tensors.size() : 0);
    return gg_graph_run(key, (hipStream_t)stream, body);
}
