// Graph executor behind the C ABI (include/bayesnn_fpga_amd.h).
//
// What it replaces in the reference: the Python T-loop of FullAnalysis._get_output
// (SA/train/results_analyzer.py:236-248) around ResNet18MCEarlyExit.forward
// (SA/models/resnet18/resnet18.py:302-346).  Instead of T sequential full-model forwards it
//   1. marks every tensor that does not depend on a stochastic site as DETERMINISTIC and runs
//      that prefix once per batch (the reference's own cost model assumes exactly this split,
//      results_analyzer.py:632-637);
//   2. folds `chunk` Monte-Carlo samples into the GEMM M dimension of every suffix op
//      (image index n = t_local * B + b), so weights are read once per chunk;
//   3. accumulates softmax moments per exit in float64 on the device.
// Activation buffers live in ONE caller-owned workspace; the suffix tensors are packed by live range (first-fit): 7 GB of
// the 288 GB for the bench's 25 500-image-sample chunk (large chunks won every A/B, so activations do round-trip HBM).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "conv_epilogue.h"
#include "kernels.h"

namespace {

struct TensorInfo {
    int h = 0, w = 0, c = 0;
    bool stoch = false;
    bool bits = false;          // holds keep bits (1 bit per element) instead of fp16 activations
    bool f32 = false;           // 4-byte elements: fp32 (output of a DENSE op; every tensor of the exact engine) or pair32 (the split engines' conv / stem / site / pool tensors)
    bool dense_out = false;     // written by a DENSE op: plain fp32 in every engine
    bool pooled_now = false;    // (run time) the producing conv of this chunk wrote fp32 means over its 4x4 map instead of the tensor
    // Lazy site (the output of an elementwise MASK op on a deterministic tensor, see bmi_create): tensors that hold the keep bits of
    // the folded batch and the deterministic input times 1/(1-p) (fp16), or -1
    int lazy_bits = -1, lazy_scaled = -1;
    bool lazy_planar_plan = false;   // (bmi_plan) ... and every one of those readers' launches passes its kernel's minimum-grid rule at the planned chunk
    bool lazy_planar = false;   // every reader is a stride-2 consumer (conv3x3_s2 on 32x32 maps / conv3x3_patch's fused shortcut) and the site draws 2 bits
                                // per element: bits + scaled copy are stored in the planar layout (kernels.h lazy_planar_off)
    bool lazy_pending = false;  // (run time) bits + scaled copy are written, the masked tensor itself is not (yet)
    bool lazy_planar_now = false;   // (run time) ... in the planar layout
    EltArgs lazy_call;          // (run time) the mask launch that materialises it on demand
    int first = -1, last = -1;  // suffix op indices (stochastic tensors only)
    size_t offset = 0;          // byte offset in the workspace
    size_t bytes = 0;           // (bmi_plan) its workspace range (stochastic tensors)
};

#define OP_MASKBITS 100   // internal: a MASK op rewritten to emit keep bits for its conv_igemm consumers

struct OpInfo {
    bmi_op_desc d;
    bool stoch = false;
    int ho = 0, wo = 0, cout = 0;
    int bits_tensor = -1;   // CONV: keep bits applied to the input while staging, or -1
    float out_mul = 1.f;    // CONV: multiplies the folded-BN scale (1/(1-p) of the input-side site)
    int nsplit = 0;         // CONV (prefix): split-K workgroups per tile (bmi_plan; 0 = none)
    bool pool_ok = false;   // CONV: its 4x4 output feeds ONE exit head and nothing else: conv3x3_s2 may write the pooled means instead
    bool pair_pool_ok = false;   // ... the same for the second conv of a pair
    bool pool_pw_ok = false;     // CONV (3x3 stride 1, 4x4 map, feeds ONE exit head only): conv3x3_pw may write the pooled means instead
    bool has_pair = false;  // CONV: a second conv on the same input rides in this launch (conv_igemm_wide pair mode)
    bmi_op_desc pair_d;
    int pair_cout = 0;
    bool has_seam = false;  // CONV (1x1 expand + residual + ReLU of a Bottleneck): the NEXT op, a plain 1x1 conv that reads this conv's output (conv1 of the
    bmi_op_desc seam_d;     // following Bottleneck), rides in this launch when conv1x1_seam takes it (else the two launches, in order)
    int seam_cout = 0;
    int64_t macs = 0;       // MACs per image (per sample in the suffix), a pair / seam partner's included
    int xstage = 0;         // (bmi_plan) the smallest exit index of any head downstream of this op's outputs (staged early exit)
};

struct ProfRec {
    int slot;
    hipEvent_t a, b;
    int family = -1;     // BMI_CONV_FAMILY_* of a conv launch
    double flops = 0;    // its algorithmic FLOPs
    double bytes = 0;    // its algorithmic HBM bytes (inputs + residual + weights once, output once)
    int out = -1;        // output tensor of the op (identifies the op in the graph)
    int images = 0;      // images (samples x batch) the launch carried
    float ms = 0.f;      // filled by bmi_profile_read
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

struct bmi_engine_s {
    BmiOptions opts;            // the process defaults at bmi_create (bmi_engine_set_option edits this copy): every entry point below runs under it
    std::vector<TensorInfo> tensors;
    std::vector<OpInfo> prefix, suffix;
    int n_exits = 0, out_dim = 0;
    int bf16 = 0;               // BMI_DTYPE_BF16
    int f32 = 0;                // fp32 activations in the workspace: BMI_DTYPE_F32 (the exact engine: fp32 conv weights, conv_exact.hip) and the split engines
    int split = 0;              // BMI_DTYPE_F16X2 (1) / BMI_DTYPE_BF16X3 (2): 16-bit head + tail weight planes, conv_split.hip
    int dtype = 0;              // BMI_DTYPE_*
    bool no_reuse = false;      // bmi_plan: every suffix tensor keeps its own workspace range ("ws_no_reuse": per-layer traces)
    int64_t prefix_macs = 0, suffix_macs = 0;
    // plan
    int max_batch = 0, chunk = 0;
    size_t ws_bytes = 0, exit_off = 0;   // exit_off: ActiveImages' region (dynamic early exit, adaptive sampling)
    size_t splitk_off = 0;               // fp32 partial sums of the split-K prefix convs
    size_t head_off = 0, head_part_bytes = 0;   // float64 partial sums of a head launch's 32-sample groups (joined in group order), one region per exit
    std::vector<std::pair<const float*, size_t>> perm;   // (bmi_plan) Masksembles tables (device pointer of the site) -> workspace offset of the permuted copy
    std::vector<float> tau;              // bmi_engine_set_temperature: the temperatures as given ([n_exits]; empty: never set = ones)
    Calibration cal;                     // the calibration map in force (kernels.h): written by the four setters below, read by make_head_args and ensemble_add
    std::vector<char> staged_ok;        // (bmi_plan) per first_exit: the staged suffix order keeps every shared workspace range's live ranges apart
    // profiling
    bool profiling = false;
    double fam_ms[BMI_CONV_FAMILIES] = {0}, fam_flops[BMI_CONV_FAMILIES] = {0}, fam_bytes[BMI_CONV_FAMILIES] = {0};
    int64_t fam_launches[BMI_CONV_FAMILIES] = {0};
    std::vector<ProfRec> recs, last;   // last: the launches of the most recent bmi_profile_read (bmi_profile_launches)
    std::vector<hipEvent_t> pool;
};

// The active images of a dynamic call (bmi_forward_mcd_exit, _exit_staged, _adaptive) and the exit region of the workspace they live in: from
// exit_off, in ints, two image lists of max_batch entries, a decide kernel's counter (64 ints), the row table of max_batch x chunk entries.
// act / rows / bc: run_op's imap / rows / Bc of the call's next launches (act null: every image is active).  A decide kernel reads act and
// writes the images that go on to next(), their number to count_dev.
struct ActiveImages {
    static size_t counter_at(size_t max_batch) { return 2 * max_batch; }
    static size_t rows_at(size_t max_batch) { return counter_at(max_batch) + 64; }
    static size_t ints(size_t max_batch, size_t rows) { return rows_at(max_batch) + rows; }
    int* lists[2];
    int *count_dev, *rows_dev;
    const int batch;
    const hipStream_t s;
    const int* act = nullptr;
    const int* rows = nullptr;
    int bc;
    int cur = 0;                    // the free list: not the one act points into
    ActiveImages(const bmi_engine_s* h, char* ws, int batch_, hipStream_t s_) : batch(batch_), s(s_), bc(batch_) {
        int* const base = (int*)(ws + h->exit_off);
        lists[0] = base; lists[1] = base + h->max_batch;
        count_dev = base + counter_at(h->max_batch);
        rows_dev = base + rows_at(h->max_batch);
    }
    int* next() const { return lists[cur]; }
    // Behind a decide kernel: how many images go on (the host's only look at the decision: one copy, one synchronise) ...
    int read_count(int* n_active) const {
        const bool ok = hipMemcpyAsync(n_active, count_dev, sizeof(int), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
        return ok ? BMI_OK : BMI_ERR_HIP;
    }
    // ... and, where the caller goes on: the list just written becomes the active one, the row table (compact image -> tensor row) is expanded
    int take(int n_active, int tc_next) {
        act = lists[cur];
        bc = n_active;
        cur ^= 1;
        rows = rows_dev;
        return launch_expand_rows(act, bc, batch, tc_next, rows_dev, s);
    }
};

SiteArgs resolve_site(const bmi_site* site, uint64_t seed, int mask_cnt0, uint64_t elem_off) {
    SiteArgs s;
    std::memset(&s, 0, sizeof(s));
    s.scale = 1.f;
    if (!site) return s;
    s.elem_off = elem_off;
    s.kind = site->kind;
    s.site_id = site->site_id;
    s.seed_lo = (uint32_t)seed;
    s.seed_hi = (uint32_t)(seed >> 32);
    if (site->kind == BMI_SITE_ELEMENTWISE || site->kind == BMI_SITE_CHANNEL) {
        s.log2_bits = bmi_site_log2_bits(site->p);
        s.thresh = bmi_drop_threshold(site->p, s.log2_bits, &s.drop_all);
        s.scale = bmi_drop_scale(site->p);
    } else if (site->kind == BMI_SITE_MASKSEMBLE) {
        s.masks = site->masks;
        s.num_masks = site->num_masks;
        s.cnt0 = mask_cnt0;
    }
    return s;
}

// Kernel selection for one conv launch: LDS-tile 3x3 patch kernel -> wide-tile per-tap implicit GEMM (Cout % 256 == 0)
// -> per-tap implicit GEMM.
// BMI_CONV_IMPL=igemm skips the patch kernel (A/B, tests).
int launch_conv(const ConvArgs& a, hipStream_t s, int* family) {
    int fam_dummy;
    if (!family) family = &fam_dummy;
    static const int mode = [] {
        const char* v = std::getenv("BMI_CONV_IMPL");
        return (v && std::strcmp(v, "igemm") == 0) ? 2 : 1;
    }();
    if (mode <= 1) {
        *family = BMI_CONV_FAMILY_PW;
        const int rcw = launch_conv3x3_pw(a, s);
        if (rcw != BMI_ERR_UNSUPPORTED) return rcw;
        *family = BMI_CONV_FAMILY_PATCH;
        const int rc = launch_conv3x3_patch(a, s);
        if (rc != BMI_ERR_UNSUPPORTED) return rc;
    }
    {
        *family = BMI_CONV_FAMILY_STREAM;
        const int rc = launch_conv1x1_stream(a, s);
        if (rc != BMI_ERR_UNSUPPORTED) return rc;
    }
    {
        *family = BMI_CONV_FAMILY_S2;
        const int rc = launch_conv3x3_s2(a, s);
        if (rc != BMI_ERR_UNSUPPORTED) return rc;
    }
    if (opt_conv_wide()) {
        *family = BMI_CONV_FAMILY_WIDE;
        const int rc = launch_conv_igemm_wide(a, s);
        if (rc != BMI_ERR_UNSUPPORTED) return rc;
    }
    *family = BMI_CONV_FAMILY_IGEMM;
    return launch_conv_igemm(a, s);
}

static bool site_ok(const bmi_site& s) {
    switch (s.kind) {
        case BMI_SITE_NONE: return true;
        case BMI_SITE_ELEMENTWISE:
        case BMI_SITE_CHANNEL: return s.p >= 0.f && s.p <= 1.f && s.site_id >= 0;
        case BMI_SITE_MASKSEMBLE: return s.num_masks > 0 && s.masks != nullptr && s.site_id >= 0;
        default: return false;
    }
}

static int shape_from_env(const char* primary, const char* fallback) {
    const char* v = std::getenv(primary);
    if (!v && fallback) v = std::getenv(fallback);
    const int x = v ? std::atoi(v) : 0;
    return x == 16 || x == 32 ? x : BMI_DEFAULT_MFMA_SHAPE;
}
static BmiOptions initial_options() {
    BmiOptions o;
    o.mfma_shape_patch = shape_from_env("BMI_MFMA_SHAPE", nullptr);
    o.mfma_shape_wide = shape_from_env("BMI_MFMA_SHAPE_WIDE", "BMI_MFMA_SHAPE");
    o.unit_dtype = BMI_DTYPE_F16;
    const char* e = std::getenv("BMI_XCD_SPLIT");
    const int x = e ? std::atoi(e) : 0;
    o.xcd_split = x == 1 || x == 2 || x == 4 ? x : 0;
    return o;
}
BmiOptions& bmi_default_options() { static BmiOptions o = initial_options(); return o; }
thread_local const BmiOptions* bmi_tl_options = nullptr;
static int unit_pair() { const int d = opt_unit_dtype(); return d == BMI_DTYPE_F16X2 ? 1 : (d == BMI_DTYPE_BF16X3 ? 2 : 0); }
static bool unit_f32act() { const int d = opt_unit_dtype(); return d == BMI_DTYPE_F32 || d == BMI_DTYPE_F16X2 || d == BMI_DTYPE_BF16X3; }

// One named switch of an option set (bmi_set_option: the process defaults; bmi_engine_set_option: one engine's snapshot).
static int set_named_option(BmiOptions& o, const char* name, int32_t value) {
    if (!name) return BMI_ERR_INVALID;
    struct Row { const char* name; int BmiOptions::*field; int lo, hi; };
    static const Row rows[] = {
        {"unit_entry_dtype", &BmiOptions::unit_dtype, BMI_DTYPE_F16, BMI_DTYPE_BF16X3},
        {"pw_persist", &BmiOptions::pw_persist, 0, 1},
        {"pw_pad_skip", &BmiOptions::pw_pad_skip, 0, 1},
        {"pw_pad_skip8", &BmiOptions::pw_pad_skip8, 0, 1},
        {"s2_pad_skip", &BmiOptions::s2_pad_skip, 0, 1},
        {"lazy_planar", &BmiOptions::lazy_planar, 0, 1},
        {"ws_no_reuse", &BmiOptions::ws_no_reuse, 0, 1},                 // read by bmi_plan
        {"wide_persist_min_x10", &BmiOptions::wide_persist_min, 10, 1000},
        {"conv_pw", &BmiOptions::conv_pw, 0, 4},
        {"conv_s2", &BmiOptions::conv_s2, 0, 2},
        {"conv_pool", &BmiOptions::conv_pool, 0, 2},
        {"mask_lazy", &BmiOptions::mask_lazy, 0, 1},
        {"conv_wide", &BmiOptions::conv_wide, 0, 1},
        {"split_shx", &BmiOptions::split_shx, 0, 2},
        {"split_tile", &BmiOptions::split_tile, 0, 1},
        {"conv_seam", &BmiOptions::conv_seam, 0, 3},                      // read by bmi_create (which ops merge) and at launch
        {"conv_stream", &BmiOptions::conv_stream, 0, 3},
        {"splitk", &BmiOptions::splitk, 0, 1},                            // read by bmi_plan
        {"dense_exact", &BmiOptions::dense_exact, 0, 1},
        {"lazy_order", &BmiOptions::lazy_order, 0, 1},
        {"epilogue_lite", &BmiOptions::epilogue_lite, 0, 2},
        {"head_batch", &BmiOptions::head_batch, 0, 1},
        {"conv_patch64", &BmiOptions::conv_patch64, 0, 1},
        {"splitk_tiles", &BmiOptions::splitk_tiles, 0, 1024},            // read by bmi_plan
        {"pair_prefix", &BmiOptions::pair_prefix, 0, 1},                  // read by bmi_create
        {"patch_direct", &BmiOptions::patch_direct, 0, 2},
    };
    for (const Row& r : rows)
        if (std::strcmp(name, r.name) == 0) {
            if (value < r.lo || value > r.hi) return BMI_ERR_INVALID;
            o.*(r.field) = value;
            return BMI_OK;
        }
    if (std::strcmp(name, "xcd_split") == 0) {
        if (value != 0 && value != 1 && value != 2 && value != 4) return BMI_ERR_INVALID;
        o.xcd_split = value;
        return BMI_OK;
    }
    const bool patch = std::strcmp(name, "mfma_shape_patch") == 0, wide = std::strcmp(name, "mfma_shape_wide") == 0;
    if (!patch && !wide) return BMI_ERR_INVALID;
    if (value != 0 && value != 16 && value != 32) return BMI_ERR_INVALID;
    (patch ? o.mfma_shape_patch : o.mfma_shape_wide) = value ? value : BMI_DEFAULT_MFMA_SHAPE;
    return BMI_OK;
}
// Channel-tile classes for xcd_tile_map: keep the weights one XCD streams under ~2.5 MB of its 4 MB L2.
int xcd_split_for(int n_ctiles, size_t weight_bytes) {
    int cs = opt_xcd_split();
    if (cs == 0) cs = weight_bytes > (8u << 20) ? 4 : (weight_bytes > (3u << 20) ? 2 : 1);
    while (cs > 1 && n_ctiles % cs != 0) cs >>= 1;
    return cs;
}

// Every tensor an op touches, with its role: f(id, role), once per operand (a tensor the op touches in two roles comes twice).  This is the
// one place that lists the operand roles; the graph passes and the plans below filter on them.  in2 and residual are a CONV's: the other
// kinds do not read the fields (add_conv refuses a STEM's residual; nothing validates a STEM's in2).  A HEAD's `out` is an exit index,
// not a tensor, and is not reported.
enum TensorRole {
    ROLE_IN = 1, ROLE_IN2 = 2, ROLE_RESIDUAL = 4, ROLE_BITS = 8, ROLE_OUT = 16, ROLE_PAIR_OUT = 32, ROLE_SEAM_OUT = 64,
    ROLE_READS = ROLE_IN | ROLE_IN2 | ROLE_RESIDUAL | ROLE_BITS
};
template <class F> void for_each_tensor(const OpInfo& op, F&& f) {
    const bmi_op_desc& d = op.d;
    f(d.in, ROLE_IN);
    if (d.kind == BMI_OP_CONV && d.in2 >= 0) f(d.in2, ROLE_IN2);
    if (d.kind == BMI_OP_CONV && d.residual >= 0) f(d.residual, ROLE_RESIDUAL);
    if (op.bits_tensor >= 0) f(op.bits_tensor, ROLE_BITS);
    if (d.kind != BMI_OP_HEAD) f(d.out, ROLE_OUT);
    if (op.has_pair) f(op.pair_d.out, ROLE_PAIR_OUT);
    if (op.has_seam) f(op.seam_d.out, ROLE_SEAM_OUT);
}
// The roles (ORed) in which op touches tensor id, 0 if it does not; it reads the tensor where roles_of(op, id) & ROLE_READS
int roles_of(const OpInfo& op, int id) {
    int r = 0;
    for_each_tensor(op, [&](int t, int role) { if (t == id) r |= role; });
    return r;
}

// Staged early exit (bmi_forward_mcd_exit_staged).  The stage of an op is the smallest exit index of any head downstream of its outputs,
// transitively; a tensor no head reads counts as the last exit's.  If op A feeds op B, every head downstream of B is also downstream of
// A, so stage(A) <= stage(B): a stable sort by stage keeps the engine's topological order.  A pair- or seam-fused op takes the smaller
// stage of its two members (the walk takes the minimum over both outputs) and runs whole there: splitting it would change the kernel
// family and so the bits.
int op_stage(const OpInfo& op, int first_exit) { return std::max(0, op.xstage - first_exit); }

// A prefix op behind a decision runs on the active images through a row table where its full-run kernel has that form; otherwise it
// runs over the whole batch (never in another kernel family: that would change the bits).  Decided under the options of the call.
// No row table: the stem, and the 1x1 convs that conv1x1_stream takes at the planned batch.
bool prefix_row_form(const bmi_engine_s* h, const OpInfo& op) {
    const bmi_op_desc& d = op.d;
    if (d.kind == BMI_OP_STEM) return false;
    if (d.kind != BMI_OP_CONV || h->f32 || d.ksize != 1 || op.has_pair || op.nsplit > 1 || d.in2 >= 0) return true;
    const TensorInfo& tin = h->tensors[d.in];
    ConvArgs a;          // the selection-relevant arguments of conv_base_args for the full-run launch (the pointers only need to be present)
    std::memset(&a, 0, sizeof(a));
    a.bf16 = h->bf16;
    a.N = a.n_ref = a.B = a.in_mod = h->max_batch;
    a.H = tin.h; a.W = tin.w; a.Cin = tin.c;
    a.Ho = op.ho; a.Wo = op.wo; a.Cout = op.cout;
    a.ksize = d.ksize; a.stride = d.stride; a.pad = d.pad; a.relu = d.relu;
    a.M = a.N * op.ho * op.wo;
    a.scale = d.scale; a.bias = d.bias;
    a.out_mul = op.out_mul;
    a.site = resolve_site(nullptr, 0, 0, 0);
    if (d.residual >= 0) { a.res = (const _Float16*)(uintptr_t)256; a.res_mod = h->max_batch; }
    return !conv1x1_stream_takes(a);
}

void plan_exit_stages(bmi_engine_s* h) {
    const int E = h->n_exits;
    std::vector<int> tmin(h->tensors.size(), E - 1);
    for (std::vector<OpInfo>* ops : {&h->suffix, &h->prefix})
        for (size_t i = ops->size(); i-- > 0;) {
            OpInfo& op = (*ops)[i];
            const bmi_op_desc& d = op.d;
            int st = d.kind == BMI_OP_HEAD ? d.out : tmin[d.out];
            if (op.has_pair) st = std::min(st, tmin[op.pair_d.out]);
            if (op.has_seam) st = std::min(st, tmin[op.seam_d.out]);
            op.xstage = st;
            for_each_tensor(op, [&](int id, int role) { if (role & ROLE_READS) tmin[id] = std::min(tmin[id], st); });
        }
    // The suffix tensors share workspace ranges by live range in the engine's order: per first_exit, the staged order must keep
    // every two tensors that share bytes live at disjoint times (where the engine's order does)
    const int n = (int)h->suffix.size(), nt = (int)h->tensors.size();
    h->staged_ok.assign(E, 0);
    for (int fe = 0; fe < E; ++fe) {
        std::vector<int> order(n);
        for (int k = 0; k < n; ++k) order[k] = k;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return op_stage(h->suffix[a], fe) < op_stage(h->suffix[b], fe); });
        std::vector<int> first(nt, -1), last(nt, -1);
        for (int k = 0; k < n; ++k)
            for_each_tensor(h->suffix[order[k]], [&](int id, int) {
                if (!h->tensors[id].stoch) return;
                if (first[id] < 0) first[id] = k;
                last[id] = k;
            });
        for (int id = 0; id < nt; ++id)
            if (h->tensors[id].lazy_bits >= 0) { first[h->tensors[id].lazy_bits] = first[id]; last[h->tensors[id].lazy_bits] = last[id]; }
        bool ok = true;
        for (int a = 1; a < nt && ok; ++a)
            for (int b = a + 1; b < nt && ok; ++b) {
                const TensorInfo &ta = h->tensors[a], &tb = h->tensors[b];
                if (!ta.stoch || !tb.stoch || ta.first < 0 || tb.first < 0 || ta.bytes == 0 || tb.bytes == 0) continue;
                if (ta.offset >= tb.offset + tb.bytes || tb.offset >= ta.offset + ta.bytes) continue;   // no shared bytes
                if (!(ta.last < tb.first || tb.last < ta.first)) continue;                              // (shared by design in the engine's order)
                ok = last[a] < first[b] || last[b] < first[a];
            }
        h->staged_ok[fe] = ok;
    }
}

namespace {

// ---- bmi_create: the descriptor's ops, one at a time, then the graph passes in the order bmi_create calls them ----------------------------

// A validated op goes to the suffix (per sample) or to the once-per-batch prefix, its MACs to that side's count
void place_op(bmi_engine_s* e, const OpInfo& op) {
    (op.stoch ? e->suffix : e->prefix).push_back(op);
    (op.stoch ? e->suffix_macs : e->prefix_macs) += op.macs;
}

// The tensor an op writes: one of the descriptor's (not the network input), written by no earlier op
bool fresh_out(const std::vector<char>& written, int id) { return id > 0 && id < (int)written.size() && !written[id]; }

int add_conv(bmi_engine_s* e, std::vector<char>& written, OpInfo op, const TensorInfo& tin) {
    const bmi_op_desc& d = op.d;
    auto tensor_ok = [&](int id) { return id >= 0 && id < (int)written.size(); };
    bool in_st = tin.stoch;
    if (!fresh_out(written, d.out) || !d.weight || d.ksize < 1 || d.stride < 1 || d.pad < 0) return BMI_ERR_INVALID;
    if ((d.kind == BMI_OP_STEM) != (d.in == 0)) return BMI_ERR_INVALID;
    if (d.site_pos != BMI_SITE_POS_OUTER && d.site_pos != BMI_SITE_POS_INNER) return BMI_ERR_INVALID;
    const bool inner = d.site_pos == BMI_SITE_POS_INNER && d.site.kind != BMI_SITE_NONE;
    if (inner && (d.in2 >= 0 || d.site.kind == BMI_SITE_MASKSEMBLE)) return BMI_ERR_UNSUPPORTED;
    const TensorInfo to = e->tensors[d.out];  // by value: the split below grows the vector
    op.ho = (tin.h + 2 * d.pad - d.ksize) / d.stride + 1;
    op.wo = (tin.w + 2 * d.pad - d.ksize) / d.stride + 1;
    op.cout = to.c;
    if (op.ho != to.h || op.wo != to.w) return BMI_ERR_INVALID;
    if (d.kind == BMI_OP_CONV && !e->f32 && (tin.c % 64 != 0 || to.c % 64 != 0)) return BMI_ERR_UNSUPPORTED;
    // the engines with fp32 activations: one generic kernel each (conv_exact / conv_split), 32-deep K-steps, 64-channel tiles
    if (d.kind == BMI_OP_CONV && e->f32 && (tin.c % 32 != 0 || to.c % 64 != 0)) return BMI_ERR_UNSUPPORTED;
    if (d.kind == BMI_OP_STEM && (to.c % 8 != 0 || to.c * d.ksize * d.ksize * tin.c > 4096 || d.residual >= 0)) return BMI_ERR_UNSUPPORTED;
    if (d.residual >= 0) {
        if (!tensor_ok(d.residual) || !written[d.residual] || d.residual == 0) return BMI_ERR_INVALID;
        const TensorInfo& tr = e->tensors[d.residual];
        if (tr.h != to.h || tr.w != to.w || tr.c != to.c) return BMI_ERR_INVALID;
        in_st = in_st || tr.stoch;
    }
    int64_t macs = (int64_t)op.ho * op.wo * op.cout * d.ksize * d.ksize * tin.c;
    if (d.kind == BMI_OP_CONV && d.in2 >= 0 && e->f32 && !e->split) return BMI_ERR_UNSUPPORTED;   // a speed feature (BN scales folded into the weights): never in the exact engine
    if (d.kind == BMI_OP_CONV && d.in2 >= 0) {
        if (!tensor_ok(d.in2) || !written[d.in2] || d.in2 == 0 || !d.weight2 || (d.scale && !e->split)) return BMI_ERR_INVALID;   // (split engines: the host's per-channel power-of-two lift comes back as `scale`)
        const TensorInfo& t2 = e->tensors[d.in2];
        if (t2.h % op.ho != 0 || t2.h / op.ho != t2.w / op.wo || t2.w % op.wo != 0) return BMI_ERR_UNSUPPORTED;
        // fp16 / bf16: conv3x3_patch / conv3x3_pw carry the shortcut; the split engines: extra K-steps of conv_split (any conv geometry)
        if (e->split ? t2.c % 32 != 0
                     : (d.ksize != 3 || d.stride != 1 || d.pad != 1 || t2.c % 64 != 0 || !conv_takes_patch_kernel(3, 1, 1, tin.c, op.cout, op.ho, op.wo)))
            return BMI_ERR_UNSUPPORTED;
        in_st = in_st || t2.stoch;
        macs += (int64_t)op.ho * op.wo * op.cout * t2.c;
    }
    op.macs = macs;
    if (!in_st && d.site.kind != BMI_SITE_NONE) {
        // deterministic conv feeding a site: keep the conv in the once-per-batch prefix
        // and apply the site while expanding to the folded sample batch.
        if (inner && d.residual >= 0) return BMI_ERR_UNSUPPORTED;
        TensorInfo tmp = to;
        tmp.stoch = false;
        e->tensors.push_back(tmp);
        const int tmp_id = (int)e->tensors.size() - 1;
        OpInfo conv = op;
        conv.d.out = tmp_id;
        conv.d.site.kind = BMI_SITE_NONE;
        conv.d.site_pos = BMI_SITE_POS_OUTER;
        conv.d.bias_post = nullptr;
        if (inner) conv.d.relu = 0;   // the prefix keeps conv*scale+bias; mask, BN shift and ReLU follow in the MASK op
        conv.stoch = false;
        place_op(e, conv);
        OpInfo m;
        std::memset(&m.d, 0, sizeof(m.d));
        m.d.kind = BMI_OP_MASK;
        m.d.in = tmp_id;
        m.d.out = d.out;
        m.d.residual = -1;
        m.d.in2 = -1;
        m.d.site = d.site;
        if (inner) { m.d.bias_post = d.bias_post; m.d.relu = d.relu; m.d.site_pos = BMI_SITE_POS_INNER; }
        m.stoch = true;
        m.ho = to.h; m.wo = to.w; m.cout = to.c;
        place_op(e, m);
        e->tensors[d.out].stoch = true;
    } else {
        op.stoch = in_st || d.site.kind != BMI_SITE_NONE;
        e->tensors[d.out].stoch = op.stoch;
        place_op(e, op);
    }
    written[d.out] = 1;
    return BMI_OK;
}

int add_mask(bmi_engine_s* e, std::vector<char>& written, OpInfo op, const TensorInfo& tin) {
    const bmi_op_desc& d = op.d;
    if (!fresh_out(written, d.out) || d.in == 0 || d.site.kind == BMI_SITE_NONE || d.site_pos != BMI_SITE_POS_OUTER) return BMI_ERR_INVALID;
    op.d.bias_post = nullptr;
    op.d.relu = 0;
    const TensorInfo& to = e->tensors[d.out];
    if (to.h != tin.h || to.w != tin.w || to.c != tin.c) return BMI_ERR_INVALID;
    if (tin.c % 8 != 0) return BMI_ERR_UNSUPPORTED;
    op.stoch = true;
    op.ho = to.h; op.wo = to.w; op.cout = to.c;
    e->tensors[d.out].stoch = true;
    place_op(e, op);
    written[d.out] = 1;
    return BMI_OK;
}

int add_maxpool(bmi_engine_s* e, std::vector<char>& written, OpInfo op, const TensorInfo& tin) {
    const bmi_op_desc& d = op.d;
    if (!fresh_out(written, d.out) || d.in == 0) return BMI_ERR_INVALID;
    const TensorInfo& to = e->tensors[d.out];
    if (to.h * 2 != tin.h || to.w * 2 != tin.w || to.c != tin.c) return BMI_ERR_INVALID;
    if (tin.c % 8 != 0) return BMI_ERR_UNSUPPORTED;
    op.stoch = tin.stoch;
    op.ho = to.h; op.wo = to.w; op.cout = to.c;
    e->tensors[d.out].stoch = tin.stoch;
    place_op(e, op);
    written[d.out] = 1;
    return BMI_OK;
}

int add_dense(bmi_engine_s* e, std::vector<char>& written, OpInfo op, const TensorInfo& tin) {
    const bmi_op_desc& d = op.d;
    if (!fresh_out(written, d.out) || d.in == 0 || !d.weight || !d.bias || d.site_pos != BMI_SITE_POS_OUTER) return BMI_ERR_INVALID;
    const TensorInfo& to = e->tensors[d.out];
    if (tin.h != 1 || tin.w != 1 || to.h != 1 || to.w != 1) return BMI_ERR_INVALID;
    if (tin.c % 32 != 0 || to.c % 64 != 0) return BMI_ERR_UNSUPPORTED;
    op.d.residual = -1; op.d.in2 = -1;
    // a site makes the layer per-sample even on a deterministic input (the layer is tiny: no conv + MASK split)
    op.stoch = tin.stoch || d.site.kind != BMI_SITE_NONE;
    op.ho = 1; op.wo = 1; op.cout = to.c;
    e->tensors[d.out].stoch = op.stoch;
    e->tensors[d.out].f32 = true;
    e->tensors[d.out].dense_out = true;
    op.macs = (int64_t)tin.c * to.c;
    place_op(e, op);
    written[d.out] = 1;
    return BMI_OK;
}

int add_head(bmi_engine_s* e, std::vector<char>& exit_seen, OpInfo op, const TensorInfo& tin) {
    const bmi_op_desc& d = op.d;
    if (d.in == 0 || d.out < 0 || d.out >= e->n_exits || exit_seen[d.out] || !d.weight || !d.bias) return BMI_ERR_INVALID;
    if (tin.c % 32 != 0) return BMI_ERR_UNSUPPORTED;   // head_fused splits K over 4 waves x 2 lane halves x float4
    if (d.site_pos == BMI_SITE_POS_INNER && d.site.kind != BMI_SITE_NONE && d.site.kind != BMI_SITE_ELEMENTWISE)
        return BMI_ERR_UNSUPPORTED;   // dropout on the logits is elementwise (F.dropout after nn.Linear)
    exit_seen[d.out] = 1;
    op.stoch = true;  // heads always run per sample (they emit per-sample softmax)
    op.cout = e->out_dim;
    op.macs = (int64_t)tin.c * e->out_dim;
    place_op(e, op);
    return BMI_OK;
}

// One op of the descriptor: validation, ho / wo / cout / macs, and its place in the prefix or the suffix (a deterministic conv that
// carries a site becomes a prefix conv and a suffix MASK op: add_conv)
int add_op(bmi_engine_s* e, std::vector<char>& written, std::vector<char>& exit_seen, const bmi_op_desc& desc_op) {
    OpInfo op;
    op.d = desc_op;
    const bmi_op_desc& d = op.d;
    if (d.in < 0 || d.in >= (int)written.size() || !written[d.in] || !site_ok(d.site)) return BMI_ERR_INVALID;
    const TensorInfo tin = e->tensors[d.in];
    if (tin.f32 && !e->f32 && d.kind != BMI_OP_DENSE && d.kind != BMI_OP_HEAD) return BMI_ERR_UNSUPPORTED;
    switch (d.kind) {
        case BMI_OP_STEM:
        case BMI_OP_CONV: return add_conv(e, written, op, tin);
        case BMI_OP_MASK: return add_mask(e, written, op, tin);
        case BMI_OP_MAXPOOL: return add_maxpool(e, written, op, tin);
        case BMI_OP_DENSE: return add_dense(e, written, op, tin);
        case BMI_OP_HEAD: return add_head(e, exit_seen, op, tin);
        default: return BMI_ERR_INVALID;
    }
}

// The descriptor into the handle: the dtype, the tensors, every op through add_op, every exit with its head
int read_graph(bmi_engine_s* e, const bmi_model_desc* desc) {
    e->n_exits = desc->n_exits;
    e->out_dim = desc->out_dim;
    e->bf16 = desc->dtype == BMI_DTYPE_BF16;
    e->split = desc->dtype == BMI_DTYPE_F16X2 ? 1 : (desc->dtype == BMI_DTYPE_BF16X3 ? 2 : 0);
    e->f32 = desc->dtype == BMI_DTYPE_F32 || e->split;
    e->dtype = desc->dtype;
    e->tensors.resize(desc->n_tensors);
    for (int i = 0; i < desc->n_tensors; ++i) {
        const bmi_tensor_desc& t = desc->tensors[i];
        if (t.h < 1 || t.w < 1 || t.c < 1) return BMI_ERR_INVALID;
        e->tensors[i].h = t.h; e->tensors[i].w = t.w; e->tensors[i].c = t.c;
        e->tensors[i].f32 = e->f32 && i > 0;   // the exact engine keeps every activation in fp32
    }
    std::vector<char> written(desc->n_tensors, 0);
    written[0] = 1;  // network input
    std::vector<char> exit_seen(desc->n_exits, 0);
    for (int k = 0; k < desc->n_ops; ++k) {
        const int rc = add_op(e, written, exit_seen, desc->ops[k]);
        if (rc != BMI_OK) return rc;
    }
    for (int x = 0; x < desc->n_exits; ++x)
        if (!exit_seen[x]) return BMI_ERR_INVALID;
    return BMI_OK;
}

// Input-side dropout: an elementwise site that expands a deterministic tensor and is consumed only
// as the input of convs that stage their input through registers (conv_igemm) is not materialised:
// the MASK op emits keep bits (16x fewer bytes), the consumers read the deterministic tensor (L2 /
// Infinity Cache resident, B images) and zero the dropped elements while staging; 1/(1-p) is
// folded into their BN scale.  Same-box A/B on the headline config: HBM traffic of the site drops
// 16x but the step time is unchanged (-0.47 ms in the mask kernel, +0.5 ms in the three consumers),
// so it is OFF by default; BMI_MASK_BITS=1 enables it (covered by the parity tests).
void rewrite_mask_bits(bmi_engine_s* e) {
    const char* env = std::getenv("BMI_MASK_BITS");
    const bool enable = env && std::atoi(env) == 1 && !e->f32;
    for (size_t mi = 0; enable && mi < e->suffix.size(); ++mi) {
        OpInfo& m = e->suffix[mi];
        if (m.d.kind != BMI_OP_MASK || m.d.site.kind != BMI_SITE_ELEMENTWISE || e->tensors[m.d.in].stoch) continue;
        if (m.d.site_pos == BMI_SITE_POS_INNER) continue;   // carries a BN shift / ReLU: must be materialised
        if (m.d.site.p >= 1.f || e->tensors[m.d.in].c % 8 != 0) continue;
        bool ok = true;
        int uses = 0;
        for (const OpInfo& c : e->suffix) {
            if (&c == &m) continue;
            const int as = roles_of(c, m.d.out) & (ROLE_IN | ROLE_RESIDUAL);      // (this pass has only ever looked at these two roles)
            if (!as) continue;
            ++uses;
            const TensorInfo& ti = e->tensors[m.d.out];
            if ((as & ROLE_RESIDUAL) || c.d.kind != BMI_OP_CONV ||
                conv_takes_patch_kernel(c.d.ksize, c.d.stride, c.d.pad, ti.c, c.cout, c.ho, c.wo))
                ok = false;
        }
        if (!ok || uses == 0) continue;
        m.d.kind = OP_MASKBITS;
        e->tensors[m.d.out].bits = true;
        for (OpInfo& c : e->suffix)
            if (&c != &m && c.d.kind == BMI_OP_CONV && c.d.in == m.d.out) {
                c.bits_tensor = m.d.out;
                c.d.in = m.d.in;
                c.out_mul = bmi_drop_scale(m.d.site.p);
            }
    }
}

// Pair fusion: two suffix convs that read the same tensor with the same geometry and a plain BN(+ReLU) epilogue
// (layerN.0.conv1 and the first conv of the exit head in front of it, resnet18.py:306/:318/:329 vs :280-299)
// run as ONE conv_igemm_wide launch: the input tile is fetched once for both and a 128-channel conv still fills
// the kernel's 256-channel tile.  The later conv moves up to the earlier one's position (it depends on nothing
// in between).  BMI_CONV_PAIR=0 keeps them separate (A/B, tests).
void fuse_pairs(bmi_engine_s* e) {
    const char* env = std::getenv("BMI_CONV_PAIR");
    const bool enable = (!env || std::atoi(env) != 0) && (!e->f32 || e->split);      // (the exact engine's kernel has no pair mode)
    auto plain = [&](const OpInfo& c) {
        return c.d.kind == BMI_OP_CONV && !c.has_pair && c.d.residual < 0 && c.d.in2 < 0 && c.d.site.kind == BMI_SITE_NONE &&
               c.bits_tensor < 0 && c.out_mul == 1.f && c.d.scale && c.d.bias;
    };
    auto merge = [&](std::vector<OpInfo>& ops, bool prefix) {
        for (size_t i = 0; i < ops.size(); ++i) {
            if (!plain(ops[i])) continue;
            const OpInfo A = ops[i];
            const TensorInfo& ti = e->tensors[A.d.in];
            // (prefix: a conv with 256+ input channels may get a split-K launch from bmi_plan on a small batch — VGG's exit convs, 37 -> 22 us —
            //  which a pair launch does not have: those stay single.  Measured: VGG-11 on f16x2 15.0 -> 14.4 M with every prefix pair merged)
            if (prefix && ti.c >= 256) continue;
            if (conv_takes_patch_kernel(A.d.ksize, A.d.stride, A.d.pad, ti.c, A.cout, A.ho, A.wo)) continue;
            for (size_t j = i + 1; j < ops.size(); ++j) {
                const OpInfo& Bo = ops[j];
                if (!plain(Bo) || Bo.d.in != A.d.in || Bo.d.ksize != A.d.ksize || Bo.d.stride != A.d.stride ||
                    Bo.d.pad != A.d.pad || Bo.d.relu != A.d.relu)
                    continue;
                if (A.cout % 128 != 0 || !conv_takes_wide_kernel(ti.c, A.cout + Bo.cout)) continue;
                if (e->split && Bo.cout % 128 != 0) continue;
                ops[i].has_pair = true;
                ops[i].pair_d = Bo.d;
                ops[i].pair_cout = Bo.cout;
                ops[i].macs += Bo.macs;
                ops.erase(ops.begin() + (long)j);
                break;
            }
        }
    };
    if (enable) merge(e->suffix, false);
    // "pair_prefix" (round 6): the same for the once-per-batch prefix — with exit-only dropout the whole network is prefix and the pairs are
    // there: the paper's configuration 3.60-3.63 M -> 3.70-3.77 M MCD-samples/s, same box (profiles/experiments/r6_exit_only_variants.txt).
    if (enable && opt_pair_prefix() && !e->f32) merge(e->prefix, true);
}

// Seam fusion (Bottleneck nets): conv3 + BN + residual + ReLU of block k followed at once by conv1 + BN + ReLU of block k+1 on its output:
// one conv1x1_seam launch produces both tensors and the wide one is not read back (conv1x1_seam.hip).  Decided per launch in run_conv.
void fuse_seams(bmi_engine_s* e) {
    for (size_t i = 0; !e->f32 && opt_conv_seam() && i + 1 < e->suffix.size(); ++i) {
        OpInfo& A = e->suffix[i];
        const OpInfo& Bo = e->suffix[i + 1];
        auto one = [&](const OpInfo& c) {
            return c.d.kind == BMI_OP_CONV && c.stoch && !c.has_pair && c.d.in2 < 0 && c.d.site.kind == BMI_SITE_NONE && c.bits_tensor < 0 && c.out_mul == 1.f &&
                   c.d.ksize == 1 && c.d.stride == 1 && c.d.pad == 0 && c.d.scale && c.d.bias;
        };
        if (!one(A) || !one(Bo) || A.d.residual < 0 || !A.d.relu || Bo.d.residual >= 0 || Bo.d.in != A.d.out) continue;
        if (!e->tensors[A.d.in].stoch || !e->tensors[A.d.residual].stoch) continue;
        if (!conv_takes_seam_kernel(e->tensors[A.d.in].c, A.cout, Bo.cout)) continue;
        A.has_seam = true;
        A.seam_d = Bo.d;
        A.seam_cout = Bo.cout;
        A.macs += Bo.macs;
        e->suffix.erase(e->suffix.begin() + (long)i + 1);
    }
}

// The reads of tensor id over the whole graph, one per role (an op that reads it as input and residual counts twice); *heads: the
// HEAD ops among the readers
int count_readers(const bmi_engine_s* e, int id, int* heads) {
    int n = 0;
    *heads = 0;
    for (const std::vector<OpInfo>* ops : {&e->prefix, &e->suffix})
        for (const OpInfo& c : *ops) {
            for_each_tensor(c, [&](int t, int role) {
                if (t != id || !(role & ROLE_READS)) return;
                ++n;
                if (c.d.kind == BMI_OP_HEAD) ++*heads;
            });
            // Left as it was: this count has always taken a STEM for a CONV.  A STEM's residual is refused by add_conv, but nothing
            // validates its in2 (no kernel reads it), so for_each_tensor does not report it and the count still adds it here.
            if (c.d.kind == BMI_OP_STEM && c.d.in2 == id) ++n;
        }
    return n;
}

// ReLU + global average pool fused into the producing conv: a plain 3x3 stride-2 conv whose 4x4 output map feeds ONE exit head and
// nothing else (ex1conv3 / ex2conv2 / ex3conv1 of the ResNets: relu -> avg_pool2d(4) -> Linear, resnet18.py:309-314, :320-325,
// :331-335) may write fp32 means [row][Cout] instead of the map when conv3x3_s2 takes the launch (decided per launch: run_conv).
void mark_pooled_tails(bmi_engine_s* e) {
    for (std::vector<OpInfo>* ops : {&e->prefix, &e->suffix})
        for (OpInfo& c : *ops) {
            if (c.d.kind != BMI_OP_CONV || e->f32) continue;
            auto eligible = [&](const bmi_op_desc& d, int cout) {
                const TensorInfo& to = e->tensors[d.out];
                int heads = 0;
                return d.ksize == 3 && d.stride == 2 && d.pad == 1 && to.h == 4 && to.w == 4 && d.residual < 0 && d.in2 < 0 &&
                       d.site.kind == BMI_SITE_NONE && cout % 128 == 0 && count_readers(e, d.out, &heads) == 1 && heads == 1;
            };
            // ... and the last conv of the net (layer4[1].conv2: stride 1, with its residual) in front of the final head: conv3x3_pw's
            // lite epilogue does the same on its registers
            auto eligible_pw = [&](const bmi_op_desc& d, int cout) {
                const TensorInfo& to = e->tensors[d.out];
                int heads = 0;
                return d.ksize == 3 && d.stride == 1 && d.pad == 1 && to.h == 4 && to.w == 4 && d.in2 < 0 && d.relu &&
                       (d.site.kind == BMI_SITE_NONE || d.site_pos != BMI_SITE_POS_INNER) && cout % 256 == 0 && !c.has_pair &&
                       count_readers(e, d.out, &heads) == 1 && heads == 1;
            };
            c.pool_pw_ok = c.bits_tensor < 0 && eligible_pw(c.d, c.cout);
            c.pool_ok = c.bits_tensor < 0 && eligible(c.d, c.cout);
            c.pair_pool_ok = c.has_pair && eligible(c.pair_d, c.pair_cout);
        }
}

// live ranges of the stochastic tensors over the suffix
void compute_live_ranges(bmi_engine_s* e) {
    for (int k = 0; k < (int)e->suffix.size(); ++k)
        for_each_tensor(e->suffix[k], [&](int id, int) {
            TensorInfo& t = e->tensors[id];
            if (!t.stoch) return;
            if (t.first < 0) t.first = k;
            t.last = k;
        });
}

// Lazy sites.  The first elementwise site of a "block"-dropout ResNet expands the once-per-batch prefix (B images) to the folded
// batch: 3.3 GB written by the MASK op and read back by its consumers on the headline config.  Where a consumer can apply the
// mask itself — conv3x3_s2 on 32x32 maps (clears the dropped elements of its patch pieces in LDS), conv3x3_patch for the input of
// a fused shortcut on 16x16 maps — the op writes the keep bits (1/16 of the bytes) and ONE scaled copy of the B images
// instead; kept x 1/(1-p) rounded to fp16 and ANDed with the bits is what the MASK op itself stores, so the result is bit for
// bit the materialised one.  Decided per launch (run_op, run_conv): a consumer whose kernel does not take the launch makes the
// MASK op's own launch happen first ("mask_lazy" = 0: always).
void plan_lazy_sites(bmi_engine_s* e) {
    for (size_t mi = 0; mi < e->suffix.size() && !e->f32; ++mi) {
        const bmi_op_desc md = e->suffix[mi].d;
        if (md.kind != BMI_OP_MASK || md.site.kind != BMI_SITE_ELEMENTWISE || md.site_pos == BMI_SITE_POS_INNER || md.site.p >= 1.f) continue;
        const TensorInfo ti = e->tensors[md.in];
        if (ti.stoch || ti.c % 32 != 0) continue;
        // every reader must be able to apply the bits itself (else the tensor is written anyway and the bits are extra work):
        //   conv3x3_s2 on 32x32 maps (also as a pair launch); conv3x3_patch for the input of a fused shortcut on 16x16 maps;
        //   1x1 convs (conv1x1_stream clears the elements in LDS, conv_igemm while staging) and the 3x3 stride-2 convs that run in
        //   conv_igemm anyway (ResNet-50's first site: 256 -> 128 k3s2, 256 -> 128 k1, 256 -> 512 k1s2).  A 3x3 stride-1 reader would
        //   lose its patch kernel to the per-tap one: not lazy.
        int readers = 0;
        bool all = true, all_s2 = true;
        for (const OpInfo& c : e->suffix) {
            const int as = roles_of(c, md.out) & ROLE_READS;      // how c reads the masked tensor
            if (!as || &c == &e->suffix[mi]) continue;
            ++readers;
            bool ok = false;
            // (round 6) conv3x3_patch's 64-channel tile — 3x3 stride-1 convs with Cout % 128 == 64 on 32-wide maps: the BasicBlocks behind the stem, which is
            // where the first "layer" site sits — clears the dropped elements of its input patch in LDS and of a residual where it is added
            auto p64 = [&](const OpInfo& q) {
                const TensorInfo& qi = e->tensors[q.d.in];
                return opt_conv_patch64() && q.d.kind == BMI_OP_CONV && !q.has_pair && q.d.in2 < 0 && q.d.ksize == 3 && q.d.stride == 1 && q.d.pad == 1 &&
                       qi.c % 64 == 0 && q.cout % 64 == 0 && q.cout % 128 != 0 && q.wo == 32 && q.ho % 8 == 0 && q.bits_tensor < 0;
            };
            if (p64(c) && !(as & ROLE_IN2)) {
                // as the input (any epilogue), and / or as the residual (the register-form epilogue: no site or the 2-bit elementwise one, outer)
                const bool res_ok = !(as & ROLE_RESIDUAL) ||
                                    (c.d.site_pos != BMI_SITE_POS_INNER && (c.d.site.kind == BMI_SITE_NONE ||
                                                                            (c.d.site.kind == BMI_SITE_ELEMENTWISE && bmi_site_log2_bits(c.d.site.p) == 1 && c.d.site.p < 1.f)));
                if (res_ok) { all = all && true; all_s2 = false; continue; }
            }
            if (c.d.kind == BMI_OP_CONV && !(as & ROLE_RESIDUAL) && c.bits_tensor < 0) {
                if (as & ROLE_IN2) { ok = !(as & ROLE_IN) && c.ho == 16 && c.wo == 16; all_s2 = all_s2 && ti.h == 2 * c.ho && ti.w == 2 * c.wo; }
                else if (c.d.in2 < 0) {
                    const bool s2 = ti.h == 32 && ti.w == 32 && c.d.residual < 0 && c.d.site.kind == BMI_SITE_NONE &&
                                    conv_takes_s2_kernel(c.d.ksize, c.d.stride, c.d.pad, ti.c, c.cout + (c.has_pair ? c.pair_cout : 0), ti.h, ti.w, c.ho, c.wo);
                    const bool igemm = !c.has_pair && ti.c % 64 == 0 && c.cout % 64 == 0 &&
                                       (c.d.ksize == 1 || (c.d.ksize == 3 && c.d.stride == 2));
                    ok = s2 || igemm;
                    all_s2 = all_s2 && s2;
                }
            }
            all = all && ok;
        }
        if (!all || readers == 0) continue;
        TensorInfo tb = ti, tsc = ti;
        tb.stoch = true; tb.bits = true; tb.first = e->tensors[md.out].first; tb.last = e->tensors[md.out].last;
        tsc.stoch = false; tsc.first = tsc.last = -1;
        e->tensors.push_back(tb);
        e->tensors.push_back(tsc);
        e->tensors[md.out].lazy_bits = (int)e->tensors.size() - 2;
        e->tensors[md.out].lazy_scaled = (int)e->tensors.size() - 1;
        e->tensors[md.out].lazy_planar = all_s2 && ti.c % 64 == 0 && ti.w >= 2 && (ti.w & (ti.w - 1)) == 0 && ((ti.h * ti.w) & (ti.h * ti.w - 1)) == 0 &&
                                         bmi_site_log2_bits(md.site.p) == 1;
    }
}

// ---- bmi_plan: the workspace, region by region in the order bmi_plan calls them (each returns where the next region starts) ----------------

// The deterministic tensors (one copy per image of the batch), from offset 0
size_t place_deterministic_tensors(bmi_engine_s* h, size_t B) {
    size_t off = 0;
    for (size_t i = 1; i < h->tensors.size(); ++i) {
        TensorInfo& t = h->tensors[i];
        if (t.stoch) continue;
        t.offset = off;
        off += align_up(B * t.h * t.w * t.c * (t.f32 ? 4 : 2), 256);
    }
    return off;
}

// first-fit packing of the suffix tensors by live range ("ws_no_reuse": no range is given out twice)
size_t pack_suffix_tensors(bmi_engine_s* h, size_t NS, size_t st_base) {
    struct Blk { size_t off, size; int last; };
    std::vector<Blk> live;
    std::vector<int> order;
    for (size_t i = 1; i < h->tensors.size(); ++i)
        if (h->tensors[i].stoch && h->tensors[i].first >= 0) order.push_back((int)i);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return h->tensors[a].first < h->tensors[b].first; });
    size_t st_peak = 0;
    h->no_reuse = opt_ws_no_reuse() != 0;
    for (int id : order) {
        TensorInfo& t = h->tensors[id];
        if (!h->no_reuse) live.erase(std::remove_if(live.begin(), live.end(), [&](const Blk& b) { return b.last < t.first; }), live.end());
        std::sort(live.begin(), live.end(), [](const Blk& a, const Blk& b) { return a.off < b.off; });
        const size_t size = align_up(t.bits ? NS * t.h * t.w * t.c / 8 : NS * t.h * t.w * t.c * (t.f32 ? 4 : 2), 256);
        size_t pos = 0;
        for (const Blk& b : live) {
            if (pos + size <= b.off) break;
            pos = std::max(pos, b.off + b.size);
        }
        t.offset = st_base + pos;
        t.bytes = size;
        live.push_back({pos, size, t.last});
        st_peak = std::max(st_peak, pos + size);
    }
    return st_base + st_peak;
}

// Split-K for the skinny deterministic 3x3 convs (VGG's 512 -> 512 convs on 2x2 maps: 250 images are 1000 pixels = 32 tiles
// of 128 x 128 on 256 CUs, 65 us at 73 TFLOP/s): one workgroup per (tile, tap), fp32 partial sums, a finishing pass.
// Decided here from the shape and the planned batch only.  Returns the bytes of the partial sums (the largest op's).
size_t plan_splitk(bmi_engine_s* h, size_t B) {
    size_t sk_bytes = 0;
    for (OpInfo& op : h->prefix) {
        op.nsplit = 0;
        const bmi_op_desc& d = op.d;
        if (d.kind != BMI_OP_CONV || (h->f32 && !h->split) || !opt_splitk() || d.ksize != 3 || d.residual >= 0 || d.in2 >= 0 || d.site.kind != BMI_SITE_NONE ||
            op.has_pair || op.bits_tensor >= 0 || op.cout % 128 != 0)
            continue;
        const TensorInfo& ti = h->tensors[d.in];
        const size_t M = B * op.ho * op.wo;
        if (h->split) {
            // the split engines (conv_split: 256-pixel tiles, 64-channel tiles on small grids): enough contiguous K ranges per tile for two
            // workgroups per CU (256 CUs), nine at most, four at least (three ranges of a 252-workgroup launch measured slower: 85 -> 110 us);
            // 72 K-steps (Cin = 256) or more
            const size_t blocks = (M + 255) / 256 * (op.cout / 64);
            const int ns = (int)std::min<size_t>(9, (512 + blocks - 1) / blocks);
            if (ti.c < 256 || ns < 4) continue;
            op.nsplit = ns;
            sk_bytes = std::max(sk_bytes, align_up((size_t)op.nsplit * M * op.cout * sizeof(float), 256));
            continue;
        }
        const size_t tiles = (M + 127) / 128 * (op.cout / 128);
        if (ti.c % 64 != 0 || ti.c < 256 || tiles > (size_t)opt_splitk_tiles()) continue;      // stride 1 or 2 (VGG-19's 256 -> 512 exit convs: 37 -> 22 us); at
                                                                       // Cin = 128 (18 K-steps) the split measured slower: 23 -> 28 us
        op.nsplit = 9;
        sk_bytes = std::max(sk_bytes, align_up((size_t)op.nsplit * M * op.cout * sizeof(float), 256));
    }
    return sk_bytes;
}

// The permuted copies of the Masksembles tables, one per distinct table of the graph
size_t place_mask_tables(bmi_engine_s* h, size_t off) {
    h->perm.clear();
    for (const std::vector<OpInfo>* ops : {&h->prefix, &h->suffix})
        for (const OpInfo& op : *ops) {
            const bmi_site& st = op.d.site;
            if (st.kind != BMI_SITE_MASKSEMBLE) continue;
            bool seen = false;
            for (const auto& pr : h->perm) seen = seen || pr.first == st.masks;
            if (seen) continue;
            const int width = op.d.kind == BMI_OP_HEAD ? h->tensors[op.d.in].c : op.cout;       // a site's table is [M][channels of its tensor]
            h->perm.push_back({st.masks, off});
            off += align_up((size_t)st.num_masks * width * sizeof(float), 256);
        }
    return off;
}

// A lazy site keeps its PLANAR layout only while every stride-2 reader's launch passes conv3x3_s2's minimum-grid rule at the planned
// full chunk (n_ref = max_batch x chunk: what the launcher looks at; 256 CUs): a reader that declines makes run_conv materialise the
// tensor — correct either way, but the planar bits + copy would then have been written for nothing (and conv_igemm / conv1x1_stream
// refuse a planar operand).  Small engines (tests, T = 1 mirrors) therefore plan NHWC lazy sites.
void plan_lazy_layout(bmi_engine_s* h, size_t NS) {
    for (TensorInfo& t : h->tensors) {
        t.lazy_planar_plan = t.lazy_planar;
        if (!t.lazy_planar) continue;
        const int id = (int)(&t - h->tensors.data());
        for (const OpInfo& c : h->suffix) {
            if (c.d.kind != BMI_OP_CONV || c.d.in != id || c.d.in2 >= 0) continue;       // (the fused-shortcut reader is conv3x3_patch: no grid rule on the operand)
            const int cout = c.cout + (c.has_pair ? c.pair_cout : 0);
            const long imgs = std::max(1, 256 / (c.ho * c.wo));
            const long tiles = ((long)NS + imgs - 1) / imgs * (cout / (cout % 256 ? 128 : 256));
            if (opt_conv_s2() != 2 && tiles < 3 * 256 / 4) t.lazy_planar_plan = false;
            if (opt_conv_s2() == 0) t.lazy_planar_plan = false;
        }
    }
}

}  // namespace

extern "C" {

int bmi_version(void) { return BMI_VERSION; }

int bmi_set_option(const char* name, int32_t value) { return set_named_option(bmi_default_options(), name, value); }

const char* bmi_error_string(int code) {
    switch (code) {
        case BMI_OK: return "ok";
        case BMI_ERR_INVALID: return "invalid argument or descriptor";
        case BMI_ERR_NOMEM: return "workspace too small";
        case BMI_ERR_HIP: return "HIP runtime / launch failure";
        case BMI_ERR_UNSUPPORTED: return "shape not supported by the gfx950 kernels";
        default: return "unknown error";
    }
}

int bmi_create(const bmi_model_desc* desc, bmi_handle* out) {
    if (!desc || !out || desc->n_tensors < 2 || desc->n_ops < 1 || !desc->tensors || !desc->ops) return BMI_ERR_INVALID;
    if (desc->n_exits < 1 || desc->out_dim < 1) return BMI_ERR_INVALID;
    if (desc->out_dim > 128) return BMI_ERR_UNSUPPORTED;
    if (desc->dtype < BMI_DTYPE_F16 || desc->dtype > BMI_DTYPE_BF16X3) return BMI_ERR_INVALID;
    std::unique_ptr<bmi_engine_s> e(new (std::nothrow) bmi_engine_s());
    if (!e) return BMI_ERR_NOMEM;
    e->opts = bmi_default_options();
    BmiOptionScope opt_scope(&e->opts);
    const int rc = read_graph(e.get(), desc);
    if (rc != BMI_OK) return rc;
    rewrite_mask_bits(e.get());
    fuse_pairs(e.get());            // after rewrite_mask_bits: a conv that reads keep bits is not "plain"
    fuse_seams(e.get());            // after fuse_pairs: an op that has a pair takes no seam
    mark_pooled_tails(e.get());     // after the fusions: reads has_pair / pair_d and counts the readers that are left
    compute_live_ranges(e.get());   // over the suffix in its final order
    plan_lazy_sites(e.get());       // last: copies first / last of the live ranges and must see the pair-fused consumers
    *out = e.release();
    return BMI_OK;
}

int bmi_engine_set_option(bmi_handle h, const char* name, int32_t value) {
    if (!h) return BMI_ERR_INVALID;
    return set_named_option(h->opts, name, value);
}

// One temperature per exit (host pointer), or NULL: off.  All ones is off too — the heads then run the untempered instantiations, and the
// outputs are the bits of an engine that never had a temperature.  Read at launch time: captured graphs keep what was set at capture.
int bmi_engine_set_temperature(bmi_handle h, const float* tau, int32_t n_exits) {
    if (!h) return BMI_ERR_INVALID;
    if (!tau) { h->tau.clear(); h->cal.inv_tau.clear(); return BMI_OK; }
    if (n_exits != h->n_exits) return BMI_ERR_INVALID;
    Calibration next = h->cal;
    if (!next.set_tau(tau, n_exits)) return BMI_ERR_INVALID;
    bool ones = true;
    for (int i = 0; i < n_exits; ++i) ones = ones && tau[i] == 1.f;
    if (ones) next.inv_tau.clear();
    if (next.check() != BMI_OK) return BMI_ERR_INVALID;             // a vector / matrix scaling is in force: clear it first
    h->tau.assign(tau, tau + n_exits);
    h->cal = next;
    return BMI_OK;
}

// The weights of the exit ensembles (caller-owned device buffer, used as given), or NULL: off — the launches are then the unweighted
// instantiations and every output keeps its bits.  Read at launch time: captured graphs keep what was set at capture.
int bmi_engine_set_ensemble_weights(bmi_handle h, const double* W_device, int32_t n_exits) {
    if (!h) return BMI_ERR_INVALID;
    if (!W_device) { h->cal.ens_w = nullptr; return BMI_OK; }
    if (n_exits != h->n_exits) return BMI_ERR_INVALID;
    h->cal.ens_w = W_device;
    return BMI_OK;
}

// Per-class scale and bias of every exit (caller-owned device arrays, used as given), or scale_device NULL: off — the heads and the ensemble
// launches are then the instantiations they were and every output keeps its bits.  Read at launch time: captured graphs keep what was set
// at capture.  Refused while a temperature other than all ones is in force (and bmi_engine_set_temperature refuses one while this is set).
int bmi_engine_set_vector_scaling(bmi_handle h, const float* scale_device, const float* bias_device, int32_t n_exits, int32_t out_dim) {
    if (!h) return BMI_ERR_INVALID;
    if (!scale_device) { h->cal.vec_scale = h->cal.vec_bias = nullptr; return BMI_OK; }
    if (n_exits != h->n_exits || out_dim != h->out_dim) return BMI_ERR_INVALID;
    Calibration next = h->cal;
    next.vec_scale = scale_device;
    next.vec_bias = bias_device;
    if (next.check() != BMI_OK) return BMI_ERR_INVALID;             // no bias, or another map is in force
    h->cal = next;
    return BMI_OK;
}

// A full [C][C] matrix and a bias per exit (caller-owned device arrays, used as given), or matrix_device NULL: off — the heads and the
// ensemble launches are then the instantiations they were and every output keeps its bits.  Read at launch time: captured graphs keep what
// was set at capture.  Refused while a temperature other than all ones or a vector scaling is in force (and both refuse while this is set).
int bmi_engine_set_matrix_scaling(bmi_handle h, const float* matrix_device, const float* bias_device, int32_t n_exits, int32_t out_dim) {
    if (!h) return BMI_ERR_INVALID;
    if (!matrix_device) { h->cal.mat = h->cal.mat_bias = nullptr; return BMI_OK; }
    if (n_exits != h->n_exits || out_dim != h->out_dim) return BMI_ERR_INVALID;
    Calibration next = h->cal;
    next.mat = matrix_device;
    next.mat_bias = bias_device;
    if (next.check() != BMI_OK) return BMI_ERR_INVALID;             // no bias, or another map is in force
    h->cal = next;
    return BMI_OK;
}

int bmi_engine_get_temperature(bmi_handle h, float* tau, int32_t capacity) {
    if (!h || !tau || capacity < h->n_exits) return BMI_ERR_INVALID;
    for (int i = 0; i < h->n_exits; ++i) tau[i] = h->tau.empty() ? 1.f : h->tau[i];
    return BMI_OK;
}

int bmi_destroy(bmi_handle h) {
    if (!h) return BMI_ERR_INVALID;
    for (auto& r : h->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto& ev : h->pool) (void)hipEventDestroy(ev);
    delete h;
    return BMI_OK;
}

int bmi_plan(bmi_handle h, int32_t max_batch, int32_t chunk_samples, size_t* workspace_bytes) {
    if (!h || max_batch < 1 || chunk_samples < 1 || !workspace_bytes) return BMI_ERR_INVALID;
    BmiOptionScope opt_scope(&h->opts);
    const size_t B = (size_t)max_batch, NS = (size_t)max_batch * chunk_samples;
    for (const TensorInfo& t : h->tensors)  // pixel indices (N * H * W) stay inside int32 (checked before the handle is touched: a refused plan leaves the last one in force)
        if (NS * t.h * t.w >= 0x7fffffffull) return BMI_ERR_UNSUPPORTED;
    size_t off = place_deterministic_tensors(h, B);
    off = pack_suffix_tensors(h, NS, off);
    h->exit_off = off;
    off += align_up(ActiveImages::ints(max_batch, NS) * sizeof(int), 256);
    h->splitk_off = off;
    off += plan_splitk(h, B);
    h->head_off = off;
    // [groups][3][B][C] moment partials + [groups][B] entropy partials (bmi_forward_mcd_entropy)
    h->head_part_bytes = align_up((size_t)((chunk_samples + 31) / 32) * max_batch * (3 * h->out_dim + 1) * sizeof(double), 256);
    off += h->head_part_bytes * (size_t)h->n_exits;      // one region per exit: the heads of a batched launch (launch_head_fused_multi) run concurrently
    off = place_mask_tables(h, off);
    h->ws_bytes = off;
    h->max_batch = max_batch;
    h->chunk = chunk_samples;
    plan_lazy_layout(h, NS);
    plan_exit_stages(h);            // after pack_suffix_tensors: checks the staged orders against the offsets just given out
    *workspace_bytes = off;
    return BMI_OK;
}

int bmi_tensor_info(bmi_handle h, int32_t id, int64_t* offset, int32_t* elem_bytes, int32_t* per_sample, int32_t* th, int32_t* tw, int32_t* tc) {
    if (!h || id < 1 || id >= (int32_t)h->tensors.size() || h->max_batch == 0) return BMI_ERR_INVALID;
    const TensorInfo& t = h->tensors[id];
    if (t.bits || (t.stoch && t.first < 0)) return BMI_ERR_UNSUPPORTED;   // keep bits / a tensor nothing reads have no activation layout
    if (offset) *offset = (int64_t)t.offset;
    if (elem_bytes) *elem_bytes = t.f32 ? 4 : 2;
    if (per_sample) *per_sample = (t.stoch ? 1 : 0) | ((h->split && !t.dense_out) ? 2 : 0);
    if (th) *th = t.h;
    if (tw) *tw = t.w;
    if (tc) *tc = t.c;
    return BMI_OK;
}

int bmi_query(bmi_handle h, int64_t* prefix_macs, int64_t* suffix_macs, int32_t* n_prefix_ops, int32_t* n_suffix_ops) {
    if (!h) return BMI_ERR_INVALID;
    if (prefix_macs) *prefix_macs = h->prefix_macs;
    if (suffix_macs) *suffix_macs = h->suffix_macs;
    if (n_prefix_ops) *n_prefix_ops = (int32_t)h->prefix.size();
    if (n_suffix_ops) *n_suffix_ops = (int32_t)h->suffix.size();
    return BMI_OK;
}

int bmi_query_op_stages(bmi_handle h, int32_t first_exit, int32_t capacity, int32_t* count, int32_t* out, int32_t* stage, int32_t* whole_batch) {
    if (!h || !count || capacity < 0 || h->max_batch == 0 || first_exit < 0 || first_exit >= h->n_exits) return BMI_ERR_INVALID;
    BmiOptionScope opt_scope(&h->opts);
    int n = 0;
    for (const std::vector<OpInfo>* ops : {&h->prefix, &h->suffix})
        for (const OpInfo& op : *ops) {
            if (op.d.kind == OP_MASKBITS) continue;
            const int k = op_stage(op, first_exit);
            const int wb = (ops == &h->prefix && k > 0 && !prefix_row_form(h, op)) ? 1 : 0;
            const int outs[3] = {op.d.kind == BMI_OP_HEAD ? -1 - op.d.out : op.d.out, op.has_pair ? op.pair_d.out : -1, op.has_seam ? op.seam_d.out : -1};
            for (int j = 0; j < 3; ++j) {
                if (j > 0 && outs[j] < 0) continue;
                if (n < capacity) {
                    if (out) out[n] = outs[j];
                    if (stage) stage[n] = k;
                    if (whole_batch) whole_batch[n] = wb;
                }
                ++n;
            }
        }
    *count = n;
    return capacity > 0 && capacity < n ? BMI_ERR_INVALID : BMI_OK;
}

int bmi_query_exit_stages(bmi_handle h, int32_t first_exit, int32_t capacity, int32_t* n_stages, int64_t* prefix_macs, int64_t* suffix_macs,
                          int32_t* n_ops, int64_t* whole_batch_macs, int32_t* n_whole_batch_ops) {
    if (!h || !n_stages || capacity < 0) return BMI_ERR_INVALID;
    if (h->max_batch == 0 || first_exit < 0 || first_exit >= h->n_exits) return BMI_ERR_INVALID;
    BmiOptionScope opt_scope(&h->opts);
    const int ns = h->n_exits - first_exit;
    *n_stages = ns;
    if (capacity == 0) return BMI_OK;
    if (capacity < ns) return BMI_ERR_INVALID;
    for (int k = 0; k < ns; ++k) {
        if (prefix_macs) prefix_macs[k] = 0;
        if (suffix_macs) suffix_macs[k] = 0;
        if (n_ops) n_ops[k] = 0;
        if (whole_batch_macs) whole_batch_macs[k] = 0;
        if (n_whole_batch_ops) n_whole_batch_ops[k] = 0;
    }
    for (const OpInfo& op : h->prefix) {
        const int k = op_stage(op, first_exit);
        if (prefix_macs) prefix_macs[k] += op.macs;
        if (n_ops) n_ops[k] += 1;
        if (k > 0 && !prefix_row_form(h, op)) {        // behind a decision but over the whole batch
            if (whole_batch_macs) whole_batch_macs[k] += op.macs;
            if (n_whole_batch_ops) n_whole_batch_ops[k] += 1;
        }
    }
    for (const OpInfo& op : h->suffix) {
        const int k = op_stage(op, first_exit);
        if (suffix_macs) suffix_macs[k] += op.macs;
        if (n_ops) n_ops[k] += 1;
    }
    return BMI_OK;
}

}  // extern "C"

namespace {

struct ProfScope {
    bmi_engine_s* e;
    hipStream_t s;
    ProfRec r;
    bool on;
    ProfScope(bmi_engine_s* e_, int slot, hipStream_t s_) : e(e_), s(s_), on(e_->profiling) {
        if (!on) return;
        auto get = [&]() {
            hipEvent_t ev;
            if (!e->pool.empty()) { ev = e->pool.back(); e->pool.pop_back(); }
            else (void)hipEventCreate(&ev);
            return ev;
        };
        r.slot = slot; r.a = get(); r.b = get();
        (void)hipEventRecord(r.a, s);
    }
    void tag(int family, double flops, double bytes) { r.family = family; r.flops = flops; r.bytes = bytes; }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(r.b, s);
        e->recs.push_back(r);
    }
};

// One forward call: built on the stack by each bmi_forward_* entry point; nothing a call does is kept in the handle.
struct Pass {
    const float* x;
    char* ws;
    hipStream_t stream;
    int B;                            // the call's batch
    uint64_t seed;
    int cnt0;
    int b0 = 0;                       // batch index of the call's image 0 (bmi_forward_mcd_images / _entropy), else 0
    double *S1 = nullptr, *S2 = nullptr, *SL = nullptr;   // [E][B][C] moment sums, or null: the heads write per-sample logits only
    double* SH = nullptr;             // bmi_forward_mcd_entropy: [E][B] sums of the per-sample entropies, or null
    float* logits = nullptr;          // bmi_forward_mcd_samples: [t - logits_t_begin][E][B][C] per-sample logits, or null
    int logits_t_begin = 0;
    bool permuted = false;            // bmi_forward_mcd_samples: a site's mask of sample t is row (t - mask_t_begin) % M of its PERMUTED table
    int mask_t_begin = 0;
};

// A site's arguments in this pass.  Masksembles masks walked with a stride (bmi_forward_mcd_samples): the kernels index row (cnt0 + t) % M
// of a site's table; the call has gathered table'[r] = table[(mask_cnt0 + r stride) % M] into the workspace, and cnt0' = -t_begin mod M
// makes that row (t - t_begin) % M — no kernel knows about the stride
SiteArgs pass_site(const bmi_engine_s* e, const Pass& p, const bmi_site* site, uint64_t elem_off = 0) {
    SiteArgs sa = resolve_site(site, p.seed, p.cnt0, elem_off);
    if (sa.kind == BMI_SITE_MASKSEMBLE && p.permuted)
        for (const auto& pr : e->perm)
            if (pr.first == sa.masks) {
                sa.masks = (const float*)(p.ws + pr.second);
                sa.cnt0 = (sa.num_masks - p.mask_t_begin % sa.num_masks) % sa.num_masks;
                break;
            }
    return sa;
}

// The arguments of one exit head's launch (head_fused.hip).
HeadArgs make_head_args(bmi_engine_s* e, const Pass& p, const OpInfo& op, int N, int t0, const int* imap, int Bc) {
    const bmi_op_desc& d = op.d;
    const TensorInfo& tin = e->tensors[d.in];
    const int B = p.B;
    const int n_rows = imap ? (N / Bc) * B : N;
    HeadArgs a;
    std::memset(&a, 0, sizeof(a));
    a.in = p.ws + tin.offset;
    a.in_kind = (e->split && !tin.dense_out) ? 2 + e->split        // the split engines' pair32 tensors
                : (tin.f32 || tin.pooled_now) ? 1 : (e->bf16 ? 2 : 0);      // pooled_now: fp32 means [row][K] written by the conv
    a.in_mod = tin.stoch ? n_rows : B;
    a.imap = imap; a.Bc = Bc;
    a.HW = tin.pooled_now ? 1 : tin.h * tin.w; a.K = tin.c; a.B = B; a.t0 = t0; a.tc = imap ? N / Bc : N / B;
    a.w = (const float*)d.weight; a.bias = d.bias; a.C = e->out_dim;
    const bool on_logits = d.site_pos == BMI_SITE_POS_INNER;
    const uint64_t soff = (uint64_t)p.b0 * (uint64_t)tin.c;          // (as site_off: [B, K] features, elementwise and per-channel draws alike)
    a.site = pass_site(e, p, on_logits ? nullptr : &d.site, soff);
    a.site_logits = pass_site(e, p, on_logits ? &d.site : nullptr);
    a.b0 = p.b0;
    a.inv_tau = e->cal.inv_tau.empty() ? 0.f : e->cal.inv_tau[d.out];       // 0: the untempered instantiations
    if (e->cal.vec_scale) {                                                 // this exit's [C] rows
        a.vec_scale = e->cal.vec_scale + (size_t)d.out * e->out_dim;
        a.vec_bias = e->cal.vec_bias + (size_t)d.out * e->out_dim;
    }
    if (e->cal.mat) {                                                       // this exit's [C][C] matrix and [C] bias
        a.mat = e->cal.mat + (size_t)d.out * e->out_dim * e->out_dim;
        a.mat_bias = e->cal.mat_bias + (size_t)d.out * e->out_dim;
    }
    if (p.S1) {
        const size_t eo = (size_t)d.out * B * e->out_dim;
        a.S1 = p.S1 + eo; a.S2 = p.S2 + eo; a.SL = p.SL + eo;
        if (p.SH) a.SH = p.SH + (size_t)d.out * B;     // this exit's [batch] row of the entropy sums
    }
    a.part = (double*)(p.ws + e->head_off + (size_t)d.out * e->head_part_bytes);     // this exit's own region
    if (p.logits) {            // per-sample logits of this exit: [t - t_begin][E][batch][C]
        const size_t plane = (size_t)B * e->out_dim;
        a.logits = p.logits + ((size_t)(t0 - p.logits_t_begin) * e->n_exits + d.out) * plane;
        a.logits_tstride = (size_t)e->n_exits * plane;
    }
    return a;
}

// image-partitioned launch (bmi_forward_mcd_images): element index of image 0 in the index space of a site on a tensor with
// `per_image` elements per image (elementwise) / `channels` (per-(image, channel) draws)
uint64_t site_off(const Pass& p, const bmi_site& st, size_t per_image, size_t channels) {
    return (uint64_t)p.b0 * (st.kind == BMI_SITE_CHANNEL ? channels : per_image);
}

// a lazy site's tensor (see bmi_create) is written when an op that reads it cannot apply the mask itself
bool pending(const bmi_engine_s* e, int id) { return id >= 0 && e->tensors[id].lazy_pending; }
int materialise(bmi_engine_s* e, int id, hipStream_t s) {
    if (!pending(e, id)) return BMI_OK;
    e->tensors[id].lazy_pending = false;
    return launch_mask_apply(e->tensors[id].lazy_call, s);
}

// The arguments of op's own conv launch (N / t0 / Bc / rows as in run_op; n_rows: the rows of a stochastic tensor): what run_conv starts from
ConvArgs conv_base_args(const bmi_engine_s* e, const Pass& p, const OpInfo& op, int N, int t0, int Bc, const int* rows, int n_rows) {
    const bmi_op_desc& d = op.d;
    const TensorInfo& tin = e->tensors[d.in];
    char* const ws = p.ws;
    const int B = p.B;
    ConvArgs a;
    std::memset(&a, 0, sizeof(a));
    a.bf16 = e->bf16;
    a.in = (const _Float16*)(ws + tin.offset);
    a.wgt = (const _Float16*)d.weight;
    a.scale = d.scale; a.bias = d.bias;
    a.out = (_Float16*)(ws + e->tensors[d.out].offset);
    a.N = N;
    // kernel selection looks at the PLANNED batch (x the planned chunk for suffix launches), never at this call's batch or sample
    // count: a t-shard, a partial chunk, an image share (bmi_forward_mcd_images) and a loader's smaller last batch all run the
    // kernels — and get the bits — of the full batch
    a.n_ref = (tin.stoch || (d.residual >= 0 && e->tensors[d.residual].stoch) || op.stoch) ? e->max_batch * e->chunk : e->max_batch;
    a.imap = rows; a.Bc = Bc;
    a.in_mod = tin.stoch ? n_rows : B;
    if (d.residual >= 0) {
        a.res = (const _Float16*)(ws + e->tensors[d.residual].offset);
        a.res_mod = e->tensors[d.residual].stoch ? n_rows : B;
    }
    a.H = tin.h; a.W = tin.w; a.Cin = tin.c;
    a.Ho = op.ho; a.Wo = op.wo; a.Cout = op.cout;
    a.ksize = d.ksize; a.stride = d.stride; a.pad = d.pad; a.relu = d.relu;
    a.M = N * op.ho * op.wo;
    a.B = B; a.t0 = t0;
    a.site = pass_site(e, p, &d.site, site_off(p, d.site, (size_t)op.ho * op.wo * op.cout, (size_t)op.cout));
    if (d.site_pos == BMI_SITE_POS_INNER && d.site.kind != BMI_SITE_NONE) { a.site_inner = 1; a.bias_post = d.bias_post; }
    a.out_mul = op.out_mul;
    if (d.in2 >= 0) {
        const TensorInfo& t2 = e->tensors[d.in2];
        a.in2 = (const _Float16*)(ws + t2.offset);
        a.wgt2 = (const _Float16*)d.weight2;
        a.in2_mod = t2.stoch ? n_rows : B;
        a.H2 = t2.h; a.W2 = t2.w; a.Cin2 = t2.c; a.stride2 = t2.h / op.ho;
    }
    if (op.bits_tensor >= 0) a.in_bits = (const uint8_t*)(ws + e->tensors[op.bits_tensor].offset);
    return a;
}

// Pair mode: base arguments `a` with the second conv on the same input riding in the launch (the 256-channel tile) ...
ConvArgs conv_pair_args(const bmi_engine_s* e, const Pass& p, const OpInfo& op, const ConvArgs& a) {
    ConvArgs q = a;
    q.wgt_b = (const _Float16*)op.pair_d.weight;
    q.scale_b = op.pair_d.scale; q.bias_b = op.pair_d.bias;
    q.out_b = (_Float16*)(p.ws + e->tensors[op.pair_d.out].offset);
    q.split = op.cout;
    q.Cout = op.cout + op.pair_cout;
    return q;
}

// ... and that second conv as a plain launch of its own, where no kernel takes the pair
ConvArgs conv_pair_second_args(const bmi_engine_s* e, const Pass& p, const OpInfo& op, const ConvArgs& a) {
    ConvArgs q = a;
    q.wgt = (const _Float16*)op.pair_d.weight;
    q.scale = op.pair_d.scale; q.bias = op.pair_d.bias;
    q.out = (_Float16*)(p.ws + e->tensors[op.pair_d.out].offset);
    q.Cout = op.pair_cout;
    return q;
}

// The next Bottleneck's reduce conv on the output of `a` (op.has_seam): the second conv of a conv1x1_seam launch, or a plain launch behind a's
ConvArgs conv_seam_second_args(const bmi_engine_s* e, const Pass& p, const OpInfo& op, const ConvArgs& a, int n_rows) {
    ConvArgs b;
    std::memset(&b, 0, sizeof(b));
    b.bf16 = e->bf16;
    b.in = a.out;
    b.wgt = (const _Float16*)op.seam_d.weight;
    b.scale = op.seam_d.scale; b.bias = op.seam_d.bias;
    b.out = (_Float16*)(p.ws + e->tensors[op.seam_d.out].offset);
    b.N = a.N; b.n_ref = a.n_ref; b.imap = a.imap; b.Bc = a.Bc; b.in_mod = n_rows;
    b.H = op.ho; b.W = op.wo; b.Cin = op.cout; b.Ho = op.ho; b.Wo = op.wo; b.Cout = op.seam_cout;
    b.ksize = 1; b.stride = 1; b.pad = 0; b.relu = op.seam_d.relu;
    b.M = a.M; b.B = a.B; b.t0 = a.t0;
    b.site = pass_site(e, p, nullptr);
    b.out_mul = 1.f;
    return b;
}

// A pending lazy site's tensor as an operand (in, res or in2): the scaled deterministic copy (B images) and the keep bits of the folded batch
// that stand in for it, and whether the two are stored in the planar layout
struct LazyOperand { const _Float16* scaled; const uint8_t* bits; bool planar; };
LazyOperand lazy_operand(const bmi_engine_s* e, const Pass& p, int id) {
    const TensorInfo& t = e->tensors[id];
    return {(const _Float16*)(p.ws + e->tensors[t.lazy_scaled].offset), (const uint8_t*)(p.ws + e->tensors[t.lazy_bits].offset), t.lazy_planar_now};
}

// The profile's cost model of a conv launch at `elem` bytes per element (2: fp16 / bf16, 4: pair32).  A pair partner widens Cout, a fused 1x1
// shortcut lengthens K.  Algorithmic bytes: every operand once (a deterministic one counts its B images), the output once, the weights once.
double operand_bytes(const bmi_engine_s* e, int id, int N, int B, double elem) {
    const TensorInfo& t = e->tensors[id];
    return elem * (t.stoch ? N : B) * t.h * t.w * t.c;
}
struct ConvCost { double flops, bytes; };
ConvCost conv_cost(const bmi_engine_s* e, const OpInfo& op, int N, int B, double elem) {
    const bmi_op_desc& d = op.d;
    const double cout = op.cout + (op.has_pair ? op.pair_cout : 0);
    const double k_len = (double)d.ksize * d.ksize * e->tensors[d.in].c + (d.in2 >= 0 ? e->tensors[d.in2].c : 0);
    const double pixels = (double)N * op.ho * op.wo;
    ConvCost c;
    c.flops = 2.0 * pixels * cout * k_len;
    c.bytes = operand_bytes(e, d.in, N, B, elem) + elem * pixels * cout + elem * cout * k_len;
    if (d.residual >= 0) c.bytes += operand_bytes(e, d.residual, N, B, elem);
    if (d.in2 >= 0) c.bytes += operand_bytes(e, d.in2, N, B, elem);
    return c;
}
// an operand read through a lazy site counts what such a launch actually has to move: the B scaled images + the folded batch's keep bits
double lazy_saving(const bmi_engine_s* e, int id, int N, int B) {
    const TensorInfo& t = e->tensors[id];
    return operand_bytes(e, id, N, B, 2.0) - (2.0 * B + N / 8.0) * t.h * t.w * t.c;
}

// A CONV op of run_op (its arguments; prof: the op's record).  The launch forms are tried in this order, each falling through to the next
// on BMI_ERR_UNSUPPORTED: the order is the policy.
int run_conv(bmi_engine_s* e, const Pass& p, const OpInfo& op, int N, int t0, int Bc, const int* rows, int n_rows, ProfScope& prof) {
    const bmi_op_desc& d = op.d;
    const int B = p.B;
    const hipStream_t s = p.stream;
    ConvArgs a = conv_base_args(e, p, op, N, t0, Bc, rows, n_rows);
    if (e->f32) {   // the exact / split engines: one generic kernel each (a.in / a.res / a.out hold fp32)
        if (!e->split) { prof.tag(-1, 0, 0); return launch_conv_exact(a, s); }
        const ConvCost c4 = conv_cost(e, op, N, B, 4.0);
        prof.tag(BMI_CONV_FAMILY_SPLIT, c4.flops, c4.bytes);
        if (op.nsplit > 1 && !op.stoch) {       // split-K (bmi_plan): raw fp32 partial sums per K range, then the finishing pass
            a.partial = (float*)(p.ws + e->splitk_off);
            a.nsplit = op.nsplit;
        }
        if (op.has_pair) {
            const int rcp = launch_conv_split(conv_pair_args(e, p, op, a), e->split == 2, s);
            if (rcp != BMI_ERR_UNSUPPORTED) return rcp;
            const int rc1 = launch_conv_split(a, e->split == 2, s);          // not taken: two launches
            return rc1 != BMI_OK ? rc1 : launch_conv_split(conv_pair_second_args(e, p, op, a), e->split == 2, s);
        }
        return launch_conv_split(a, e->split == 2, s);
    }
    const ConvCost c2 = conv_cost(e, op, N, B, 2.0);
    const double flops = c2.flops, bytes = c2.bytes;
    if (op.has_seam) {
        // the next Bottleneck's reduce conv on this conv's output: one conv1x1_seam launch, or the two launches in order
        const ConvArgs b = conv_seam_second_args(e, p, op, a, n_rows);
        const double flops_b = 2.0 * N * op.ho * op.wo * (double)op.seam_cout * op.cout;
        const double bytes_b = 2.0 * N * op.ho * op.wo * (double)op.seam_cout + 2.0 * (double)op.seam_cout * op.cout;   // (its input never leaves the chip)
        const int rcs = launch_conv1x1_seam(a, b, s);
        if (rcs != BMI_ERR_UNSUPPORTED) {
            prof.tag(BMI_CONV_FAMILY_SEAM, flops + flops_b, bytes + bytes_b);
            return rcs;
        }
        int fam = -1;
        const int rc1 = launch_conv(a, s, &fam);
        prof.tag(fam, flops + flops_b, bytes + bytes_b + 2.0 * N * op.ho * op.wo * (double)op.cout);
        return rc1 != BMI_OK ? rc1 : launch_conv(b, s);
    }
    if (op.has_pair) {
        const ConvArgs pr = conv_pair_args(e, p, op, a);
        e->tensors[d.out].pooled_now = e->tensors[op.pair_d.out].pooled_now = false;
        if (pending(e, d.in)) {      // lazy site on the input: conv3x3_s2 clears the dropped elements in LDS, or the tensor is written now
            ConvArgs m = pr;
            const LazyOperand v = lazy_operand(e, p, d.in);
            m.in = v.scaled; m.in_mod = B; m.in_bits = v.bits; m.lazy_planar = v.planar;
            const int rcl = launch_conv3x3_s2(m, s);
            prof.tag(BMI_CONV_FAMILY_S2, flops, bytes - lazy_saving(e, d.in, N, B));
            if (rcl != BMI_ERR_UNSUPPORTED) return rcl;
            const int rcm = materialise(e, d.in, s);
            if (rcm != BMI_OK) return rcm;
        }
        if (opt_conv_pool() && (op.pool_ok || op.pair_pool_ok)) {
            ConvArgs q = pr;         // the pooled means take the place of the map in the workspace (16 x 4 B <= 16 x 16 x 2 B per channel)
            if (op.pool_ok) q.pool = (float*)q.out;
            if (op.pair_pool_ok) q.pool_b = (float*)q.out_b;
            const int rcp = launch_conv3x3_s2(q, s);
            prof.tag(BMI_CONV_FAMILY_S2, flops, bytes);
            if (rcp != BMI_ERR_UNSUPPORTED) {
                e->tensors[d.out].pooled_now = op.pool_ok;
                e->tensors[op.pair_d.out].pooled_now = op.pair_pool_ok;
                return rcp;
            }
        }
        int rc = launch_conv3x3_s2(pr, s);
        prof.tag(BMI_CONV_FAMILY_S2, flops, bytes);
        if (rc != BMI_ERR_UNSUPPORTED) return rc;
        rc = launch_conv_igemm_wide(pr, s);
        prof.tag(BMI_CONV_FAMILY_WIDE, flops, bytes);
        if (rc != BMI_ERR_UNSUPPORTED) return rc;
        int fam = -1;
        const int rc2 = launch_conv(a, s, &fam);          // not taken after all: two plain launches
        prof.tag(fam, flops, bytes);
        return rc2 != BMI_OK ? rc2 : launch_conv(conv_pair_second_args(e, p, op, a), s);
    }
    if (pending(e, d.residual)) {    // (run_op's res_lazy_ok) the residual through its keep bits: conv3x3_patch's 64-channel tile — with the input too
        ConvArgs m = a;              //  when it is the same pending tensor or another one
        const LazyOperand r = lazy_operand(e, p, d.residual);
        m.res = r.scaled; m.res_mod = B; m.res_bits = r.bits; m.lazy_planar = r.planar;
        if (pending(e, d.in)) {
            const LazyOperand v = lazy_operand(e, p, d.in);
            m.in = v.scaled; m.in_mod = B; m.in_bits = v.bits; m.lazy_planar = v.planar || r.planar;
        }
        const int rcl = launch_conv3x3_patch(m, s);
        prof.tag(BMI_CONV_FAMILY_PATCH, flops, bytes - lazy_saving(e, d.residual, N, B) - (pending(e, d.in) ? lazy_saving(e, d.in, N, B) : 0.0));
        if (rcl != BMI_ERR_UNSUPPORTED) return rcl;
        const int rcm = materialise(e, d.residual, s);
        if (rcm != BMI_OK) return rcm;
    }
    if (pending(e, d.in)) {          // whichever kernel of the chain applies keep bits: conv1x1_stream, conv3x3_s2, conv_igemm
        ConvArgs m = a;
        const LazyOperand v = lazy_operand(e, p, d.in);
        m.in = v.scaled; m.in_mod = B; m.in_bits = v.bits; m.lazy_planar = v.planar;
        int faml = -1;
        const int rcl = launch_conv(m, s, &faml);
        prof.tag(faml, flops, bytes - lazy_saving(e, d.in, N, B));
        if (rcl != BMI_ERR_UNSUPPORTED) return rcl;
        const int rcm = materialise(e, d.in, s);
        if (rcm != BMI_OK) return rcm;
    }
    if (pending(e, d.in2)) {         // ... on the input of a fused shortcut: conv3x3_patch on 16x16 maps
        int rcl = BMI_ERR_UNSUPPORTED;
        if (op.ho == 16 && op.wo == 16) {
            ConvArgs m = a;
            const LazyOperand v = lazy_operand(e, p, d.in2);
            m.in2 = v.scaled; m.in2_mod = B; m.in2_bits = v.bits; m.lazy_planar = v.planar;
            rcl = launch_conv3x3_patch(m, s);
            prof.tag(BMI_CONV_FAMILY_PATCH, flops, bytes - lazy_saving(e, d.in2, N, B));
        }
        if (rcl != BMI_ERR_UNSUPPORTED) return rcl;
        const int rcm = materialise(e, d.in2, s);
        if (rcm != BMI_OK) return rcm;
    }
    e->tensors[d.out].pooled_now = false;
    if (op.nsplit > 1 && !op.stoch) {        // (under a row table too: conv_igemm's split-K form writes through it)
        a.partial = (float*)(p.ws + e->splitk_off);
        a.nsplit = op.nsplit;
        prof.tag(BMI_CONV_FAMILY_IGEMM, flops, bytes);
        return launch_conv_igemm(a, s);
    }
    if (opt_conv_pool() == 1 && op.pool_pw_ok) {      // ("conv_pool" = 2: conv3x3_s2's only)
        ConvArgs q = a;
        q.pool = (float*)q.out;
        const int rcp = launch_conv3x3_pw(q, s);
        if (rcp != BMI_ERR_UNSUPPORTED) {
            prof.tag(BMI_CONV_FAMILY_PW, flops, bytes);
            e->tensors[d.out].pooled_now = true;
            return rcp;
        }
    }
    if (opt_conv_pool() && op.pool_ok) {
        ConvArgs q = a;
        q.pool = (float*)q.out;
        const int rcp = launch_conv3x3_s2(q, s);
        if (rcp != BMI_ERR_UNSUPPORTED) {
            prof.tag(BMI_CONV_FAMILY_S2, flops, bytes);
            e->tensors[d.out].pooled_now = true;
            return rcp;
        }
    }
    int fam = -1;
    const int rcc = launch_conv(a, s, &fam);
    prof.tag(fam, flops, bytes);
    return rcc;
}

// imap / rows / Bc: dynamic early exit and adaptive sampling: N = samples * Bc compact images of the B-image batch; imap = the Bc
// active images (heads), rows = the N-entry row table (ConvArgs::imap, EltArgs::rows, the maxpool / dense launchers); null = all images
int run_op(bmi_engine_s* e, const Pass& p, const OpInfo& op, int N, int t0, const int* imap = nullptr, int Bc = 0, const int* rows = nullptr) {
    const bmi_op_desc& d = op.d;
    const TensorInfo& tin = e->tensors[d.in];
    char* const ws = p.ws;
    const int B = p.B;
    const hipStream_t s = p.stream;
    const int n_rows = imap ? (N / Bc) * B : N;     // rows of a stochastic tensor (original folded layout)
    if (imap && d.kind != BMI_OP_CONV && d.kind != BMI_OP_HEAD && d.kind != BMI_OP_MASK && d.kind != BMI_OP_MAXPOOL && d.kind != BMI_OP_DENSE)
        return BMI_ERR_UNSUPPORTED;      // (OP_MASKBITS: its conv_igemm readers have no row-table form)
    if (imap && e->f32 && !e->split) return BMI_ERR_UNSUPPORTED;      // (the exact engine: parity only)
    // a pending lazy operand is written now if this op cannot apply the mask itself
    // (a pending RESIDUAL stays pending only for conv3x3_patch's 64-channel tile, which masks it where it is added: tried first in run_conv)
    const bool res_lazy_ok = d.kind == BMI_OP_CONV && pending(e, d.residual) && !op.has_pair && d.in2 < 0 && d.ksize == 3 && d.stride == 1 && d.pad == 1 &&
                             op.cout % 64 == 0 && op.cout % 128 != 0 && op.wo == 32 && op.ho % 8 == 0 && opt_conv_patch64() && !imap;
    if (d.kind != BMI_OP_CONV || (pending(e, d.residual) && !res_lazy_ok) || (pending(e, d.in) && pending(e, d.in2))) {
        int rcm = materialise(e, d.in, s);
        if (rcm == BMI_OK && d.kind == BMI_OP_CONV) { rcm = materialise(e, d.residual, s); if (rcm == BMI_OK) rcm = materialise(e, d.in2, s); }
        if (rcm != BMI_OK) return rcm;
    }
    ProfScope prof(e, d.kind == OP_MASKBITS ? BMI_OP_MASK : d.kind, s);
    prof.r.out = d.out; prof.r.images = N;
    switch (d.kind) {
        case BMI_OP_STEM:
            return launch_stem_conv(p.x, (const float*)d.weight, d.scale, d.bias, (_Float16*)(ws + e->tensors[d.out].offset), N,
                                    tin.c, tin.h, tin.w, op.cout, d.ksize, d.stride, d.pad, d.relu, e->dtype, s);     // (F32: fp32 out; F16X2 / BF16X3: pair32 out)
        case BMI_OP_CONV:
            return run_conv(e, p, op, N, t0, Bc, rows, n_rows, prof);
        case OP_MASKBITS:
            return launch_mask_bits((uint8_t*)(ws + e->tensors[d.out].offset), N, tin.h * tin.w, tin.c,
                                    pass_site(e, p, &d.site, site_off(p, d.site, (size_t)tin.h * tin.w * tin.c, (size_t)tin.c)), B, t0, s);
        case BMI_OP_MASK: {
            EltArgs a;
            std::memset(&a, 0, sizeof(a));
            a.bf16 = e->bf16;
            a.in = (const _Float16*)(ws + tin.offset);
            a.out = ws + e->tensors[d.out].offset;
            a.N = N; a.in_mod = tin.stoch ? n_rows : B; a.HW = tin.h * tin.w; a.C = tin.c; a.B = B; a.t0 = t0;
            a.rows = rows;
            a.site = pass_site(e, p, &d.site, site_off(p, d.site, (size_t)tin.h * tin.w * tin.c, (size_t)tin.c));
            if (d.site_pos == BMI_SITE_POS_INNER) { a.bias_post = d.bias_post; a.relu = d.relu; }
            a.pair = e->split;                                     // the split engines: pair32 tensors in and out
            if (e->f32) return launch_mask_apply_f32(a, s);
            TensorInfo& to = e->tensors[d.out];
            to.lazy_pending = false;
            // under a row table a lazy site is materialised (its own workspace range, the lazy path's fallback): its stride-2 reader,
            // conv3x3_s2 with keep bits, has no row-table form
            if (to.lazy_bits >= 0 && opt_mask_lazy() && !tin.stoch && N % B == 0 && !rows) {
                const bool planar = to.lazy_planar_plan && opt_lazy_planar();
                to.lazy_planar_now = planar;
                const int rcb = launch_mask_bits((uint8_t*)(ws + e->tensors[to.lazy_bits].offset), N, tin.h * tin.w, tin.c, a.site, B, t0, s, planar ? tin.w : 0);
                if (rcb == BMI_OK) {
                    const int rcs = launch_scale_copy(a.in, (_Float16*)(ws + e->tensors[to.lazy_scaled].offset), (long)B * tin.h * tin.w * tin.c,
                                                      a.site.scale, e->bf16, s, planar ? tin.h * tin.w : 0, planar ? tin.w : 0, planar ? tin.c : 0);
                    if (rcs != BMI_OK) return rcs;
                    to.lazy_call = a;
                    to.lazy_pending = true;
                    return BMI_OK;
                }
                if (rcb != BMI_ERR_UNSUPPORTED) return rcb;
            }
            return launch_mask_apply(a, s);
        }
        case BMI_OP_MAXPOOL:
            if (e->f32) return launch_maxpool2_f32((const float*)(ws + tin.offset), (float*)(ws + e->tensors[d.out].offset), N, tin.h, tin.w, tin.c, s, e->split, rows);
            return launch_maxpool2((const _Float16*)(ws + tin.offset), (_Float16*)(ws + e->tensors[d.out].offset), N, tin.h,
                                   tin.w, tin.c, e->bf16, s, rows);
        case BMI_OP_DENSE:
            // input: fp32 (a dense layer's output; any tensor of the exact engine), the engine's 16-bit type, or pair32 (kinds 3 | 4)
            return launch_dense_f32(ws + tin.offset, (e->split && !tin.dense_out) ? 2 + e->split : (tin.f32 ? 1 : (e->bf16 ? 2 : 0)), (const float*)d.weight, d.bias,
                                    (float*)(ws + e->tensors[d.out].offset), N, tin.stoch ? n_rows : B, tin.c, op.cout, d.relu,
                                    pass_site(e, p, &d.site, site_off(p, d.site, (size_t)op.cout, (size_t)op.cout)), B, t0, s, rows);
        case BMI_OP_HEAD:
            // pool + site + Linear + softmax + the chunk's moment sums in one launch (head_fused.hip)
            return launch_head_fused(make_head_args(e, p, op, N, t0, imap, Bc), s);
    }
    return BMI_ERR_INVALID;
}

// One chunk of the suffix.  Consecutive exit heads run as ONE launch ("head_batch"; launch_head_fused_multi): with exit-only dropout — what
// every run of the paper uses, Software_Artifact/script_figs/journal_script.sh:10-63 — the suffix is nothing but the heads, each a launch of
// mostly fixed latency; the same arithmetic per head, the same bits.  Under a row table (imap / rows / Bc as in run_op: adaptive sampling)
// the heads run one by one.
// (run_suffix_ops: the same over ops op_at(0 .. n-1), a stage of bmi_forward_mcd_exit_staged)
template <class OpAt>
int run_suffix_ops(bmi_engine_s* e, const Pass& p, size_t n, OpAt op_at, int N, int t0, const int* imap, int Bc, const int* rows) {
    const hipStream_t s = p.stream;
    for (size_t i = 0; i < n;) {
        size_t j = i;
        if (opt_head_batch() && !imap)
            while (j < n && j - i < BMI_HEAD_PACK_MAX && op_at(j).d.kind == BMI_OP_HEAD && !e->tensors[op_at(j).d.in].lazy_pending) ++j;
        if (j - i >= 2) {
            HeadArgs list[BMI_HEAD_PACK_MAX];
            for (size_t k = i; k < j; ++k) list[k - i] = make_head_args(e, p, op_at(k), N, t0, nullptr, 0);
            int rc;
            {
                ProfScope prof(e, BMI_OP_HEAD, s);
                prof.r.out = op_at(i).d.out; prof.r.images = N;
                rc = launch_head_fused_multi(list, (int)(j - i), s);
            }
            if (rc == BMI_OK) { i = j; continue; }
            if (rc != BMI_ERR_UNSUPPORTED) return rc;
            if (e->profiling && !e->recs.empty()) {          // not taken: drop the empty record, the heads follow one by one
                e->pool.push_back(e->recs.back().a); e->pool.push_back(e->recs.back().b);
                e->recs.pop_back();
            }
        }
        const int rc = run_op(e, p, op_at(i), N, t0, imap, Bc, rows);
        if (rc != BMI_OK) return rc;
        ++i;
    }
    return BMI_OK;
}

int run_suffix(bmi_engine_s* e, const Pass& p, int N, int t0, const int* imap = nullptr, int Bc = 0, const int* rows = nullptr) {
    const std::vector<OpInfo>& ops = e->suffix;
    return run_suffix_ops(e, p, ops.size(), [&](size_t i) -> const OpInfo& { return ops[i]; }, N, t0, imap, Bc, rows);
}

// bmi_forward_mcd_ensemble: the exit-ensemble sums of the call and the caller's scratch, one chunk of per-sample logits [chunk][E][B][C]
struct EnsembleSums {
    double *Q1, *Q2, *QH;
    float* scratch;
};

// The argument check the three *_ensemble entry points share, in front of their own entry point's checks
int ensemble_args_ok(bmi_handle h, int32_t batch, const double* Q1, const double* Q2, const double* QH, const void* scratch, size_t scratch_bytes) {
    if (!h || !Q1 || !Q2 || !QH || !scratch) return BMI_ERR_INVALID;
    if (!ensemble_takes(h->n_exits, h->out_dim)) return BMI_ERR_UNSUPPORTED;
    if (h->max_batch == 0 || batch < 1 || batch > h->max_batch) return BMI_ERR_INVALID;
    if (scratch_bytes < bmi_ensemble_scratch_bytes(h, batch)) return BMI_ERR_NOMEM;
    return BMI_OK;
}

// Adds the tc samples of per-sample logits in ens.scratch ([tc][E][B][C]) to the ensemble sums, under the handle's calibration: the one
// launch_ensemble_moments call of the engine.  rows: the images (and of each its exits) the launch covers, default: all.
int ensemble_add(const bmi_engine_s* e, const EnsembleSums& ens, int tc, int B, hipStream_t s, const EnsRows& rows = EnsRows()) {
    return launch_ensemble_moments(ens.scratch, tc, e->n_exits, B, e->out_dim, e->cal, rows, ens.Q1, ens.Q2, ens.QH, s);
}

// bmi_forward_mcd_votes: the vote counts of the call (votes.hip), taken from the chunk of per-sample logits the ensemble launch reads
struct VoteCounts {
    int32_t* V;
    int32_t* nonfinite;      // or null
};

// The folded path: the prefix once, then samples t_begin .. t_begin+t_count-1 through the suffix, `chunk` at a time.
// ens: every chunk's heads also write their logits into ens->scratch (a runtime branch of the same kernels: S1 / S2 / SL / SH keep their
// bits), and one launch of ensemble.hip behind them adds the chunk's samples, in sample order, to the ensemble sums.
// votes (with ens only): one launch of votes.hip on the same scratch, under the same calibration, adds the chunk's votes.
int forward_folded(bmi_engine_s* e, const Pass& p, int t_begin, int t_count, const EnsembleSums* ens = nullptr, const VoteCounts* votes = nullptr) {
    BmiOptionScope opt_scope(&e->opts);
    for (const OpInfo& op : e->prefix) {
        const int rc = run_op(e, p, op, p.B, 0);
        if (rc != BMI_OK) return rc;
    }
    Pass pc = p;
    for (int t0 = t_begin; t0 < t_begin + t_count; t0 += e->chunk) {
        const int tc = std::min(e->chunk, t_begin + t_count - t0);
        if (ens) { pc.logits = ens->scratch; pc.logits_t_begin = t0; }
        int rc = run_suffix(e, pc, tc * p.B, t0);
        if (rc != BMI_OK) return rc;
        if (!ens) continue;
        // (no BMI_PROFILE_ENSEMBLE record here, unlike the staged and adaptive paths: the profile tables of this path never had one, and
        //  adding it is a change of what profile_launches() returns, not a refactoring)
        rc = ensemble_add(e, *ens, tc, p.B, p.stream);
        if (rc != BMI_OK) return rc;
        if (!votes) continue;
        rc = launch_vote_counts(ens->scratch, tc, e->n_exits, p.B, e->out_dim, e->cal, votes->V, votes->nonfinite, p.stream);
        if (rc != BMI_OK) return rc;
    }
    return BMI_OK;
}

// bmi_forward_mcd, _images and _entropy (SH: null but for _entropy): their argument checks, then the folded path.
int forward_moments(bmi_handle h, const float* x_nchw, int32_t batch, int32_t image_offset, int32_t t_begin, int32_t t_count, uint64_t seed,
                    int32_t mask_cnt0, double* S1, double* S2, double* SL, double* SH, void* workspace, size_t workspace_bytes, bmi_stream stream,
                    const EnsembleSums* ens = nullptr, const VoteCounts* votes = nullptr) {
    const int rco = bmi_image_offset_ok(h, image_offset);      // (a null handle: BMI_ERR_INVALID; image 0 always passes)
    if (rco != BMI_OK) return rco;
    if (!x_nchw || !S1 || !S2 || !SL || !workspace) return BMI_ERR_INVALID;
    if (batch < 1 || t_count < 1 || t_begin < 0 || mask_cnt0 < 0) return BMI_ERR_INVALID;
    if (h->max_batch == 0 || batch > h->max_batch) return BMI_ERR_INVALID;
    if (workspace_bytes < h->ws_bytes) return BMI_ERR_NOMEM;
    Pass p{x_nchw, (char*)workspace, (hipStream_t)stream, batch, seed, mask_cnt0};
    p.b0 = image_offset;
    p.S1 = S1; p.S2 = S2; p.SL = SL; p.SH = SH;
    return forward_folded(h, p, t_begin, t_count, ens, votes);
}

}  // namespace

extern "C" {

int bmi_image_offset_ok(bmi_handle h, int32_t image_offset) {
    if (!h || image_offset < 0) return BMI_ERR_INVALID;
    if (image_offset == 0) return BMI_OK;
    // a site's index offset must be a whole number of Philox calls at every bit width (64 elements): per-image element counts
    // of every site tensor — conv / mask outputs, pooled features, dense outputs
    for (const std::vector<OpInfo>* ops : {&h->prefix, &h->suffix})
        for (const OpInfo& op : *ops) {
            const bmi_op_desc& d = op.d;
            if (d.site.kind != BMI_SITE_ELEMENTWISE && d.site.kind != BMI_SITE_CHANNEL) continue;
            if (d.kind == BMI_OP_HEAD && d.site_pos == BMI_SITE_POS_INNER) continue;      // logits site: the kernel adds b0 itself
            const TensorInfo& tin = h->tensors[d.in];
            const size_t unit = d.kind == BMI_OP_HEAD ? (size_t)tin.c
                                : d.kind == BMI_OP_DENSE || d.site.kind == BMI_SITE_CHANNEL ? (size_t)op.cout
                                : (size_t)op.ho * op.wo * op.cout;
            if (((size_t)image_offset * unit) % 64 != 0) return BMI_ERR_UNSUPPORTED;
        }
    return BMI_OK;
}

int bmi_forward_mcd(bmi_handle h, const float* x_nchw, int32_t batch, int32_t t_begin, int32_t t_count, uint64_t seed,
                    int32_t mask_cnt0, double* S1, double* S2, double* SL, void* workspace, size_t workspace_bytes,
                    bmi_stream stream) {
    return forward_moments(h, x_nchw, batch, 0, t_begin, t_count, seed, mask_cnt0, S1, S2, SL, nullptr, workspace, workspace_bytes, stream);
}

int bmi_forward_mcd_images(bmi_handle h, const float* x_nchw, int32_t batch, int32_t image_offset, int32_t t_begin,
                           int32_t t_count, uint64_t seed, int32_t mask_cnt0, double* S1, double* S2, double* SL,
                           void* workspace, size_t workspace_bytes, bmi_stream stream) {
    return forward_moments(h, x_nchw, batch, image_offset, t_begin, t_count, seed, mask_cnt0, S1, S2, SL, nullptr, workspace,
                           workspace_bytes, stream);
}

int bmi_forward_mcd_entropy(bmi_handle h, const float* x_nchw, int32_t batch, int32_t image_offset, int32_t t_begin,
                            int32_t t_count, uint64_t seed, int32_t mask_cnt0, double* S1, double* S2, double* SL, double* SH,
                            void* workspace, size_t workspace_bytes, bmi_stream stream) {
    if (!h || !SH) return BMI_ERR_INVALID;
    return forward_moments(h, x_nchw, batch, image_offset, t_begin, t_count, seed, mask_cnt0, S1, S2, SL, SH, workspace,
                           workspace_bytes, stream);
}

size_t bmi_ensemble_scratch_bytes(bmi_handle h, int32_t batch) {
    if (!h || h->max_batch == 0 || batch < 1 || batch > h->max_batch) return 0;
    return (size_t)h->chunk * h->n_exits * batch * h->out_dim * sizeof(float);
}

int bmi_forward_mcd_ensemble(bmi_handle h, const float* x_nchw, int32_t batch, int32_t image_offset, int32_t t_begin, int32_t t_count,
                             uint64_t seed, int32_t mask_cnt0, double* S1, double* S2, double* SL, double* SH, double* Q1, double* Q2,
                             double* QH, void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes, bmi_stream stream) {
    if (!h || !SH) return BMI_ERR_INVALID;
    const int rce = ensemble_args_ok(h, batch, Q1, Q2, QH, scratch, scratch_bytes);
    if (rce != BMI_OK) return rce;
    const EnsembleSums ens{Q1, Q2, QH, (float*)scratch};
    return forward_moments(h, x_nchw, batch, image_offset, t_begin, t_count, seed, mask_cnt0, S1, S2, SL, SH, workspace, workspace_bytes, stream,
                           &ens);
}

int bmi_forward_mcd_votes(bmi_handle h, const float* x_nchw, int32_t batch, int32_t image_offset, int32_t t_begin, int32_t t_count, uint64_t seed,
                          int32_t mask_cnt0, double* S1, double* S2, double* SL, double* SH, double* Q1, double* Q2, double* QH, int32_t* V,
                          int32_t* nonfinite, void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes, bmi_stream stream) {
    if (!h || !SH || !V) return BMI_ERR_INVALID;
    const int rce = ensemble_args_ok(h, batch, Q1, Q2, QH, scratch, scratch_bytes);
    if (rce != BMI_OK) return rce;
    if (!vote_counts_takes(h->chunk, h->n_exits, batch, h->out_dim)) return BMI_ERR_UNSUPPORTED;
    const EnsembleSums ens{Q1, Q2, QH, (float*)scratch};
    const VoteCounts votes{V, nonfinite};
    return forward_moments(h, x_nchw, batch, image_offset, t_begin, t_count, seed, mask_cnt0, S1, S2, SL, SH, workspace, workspace_bytes, stream,
                           &ens, &votes);
}

int bmi_forward_mcd_samples(bmi_handle h, const float* x_nchw, int32_t batch, int32_t t_begin, int32_t t_count, uint64_t seed,
                            int32_t mask_cnt0, int32_t mask_stride, float* logits, double* S1, double* S2, double* SL, void* workspace,
                            size_t workspace_bytes, bmi_stream stream) {
    if (!h || !logits || !workspace || mask_stride < 1 || t_begin < 0 || mask_cnt0 < 0) return BMI_ERR_INVALID;
    BmiOptionScope opt_scope(&h->opts);
    if ((S1 || S2 || SL) && !(S1 && S2 && SL)) return BMI_ERR_INVALID;
    if (h->max_batch == 0 || batch < 1 || batch > h->max_batch) return BMI_ERR_INVALID;
    if (workspace_bytes < h->ws_bytes) return BMI_ERR_NOMEM;
    if (!x_nchw || t_count < 1) return BMI_ERR_INVALID;
    Pass p{x_nchw, (char*)workspace, (hipStream_t)stream, batch, seed, mask_cnt0};
    p.S1 = S1; p.S2 = S2; p.SL = SL;                  // (all null: per-sample logits only)
    p.logits = logits; p.logits_t_begin = t_begin;
    if ((mask_stride != 1 || t_begin != 0) && !h->perm.empty()) {
        // gather every Masksembles table in the order this call walks it: table'[r] = table[(mask_cnt0 + r * stride) % M]
        // (stride 1 from t_begin > 0 too: the kernels index (cnt0 + t) mod M with the GLOBAL sample index t, which would rotate the walk by t_begin —
        //  this call's contract is mask_cnt0 for its FIRST sample, whatever t_begin)
        for (const std::vector<OpInfo>* ops : {&h->prefix, &h->suffix})
            for (const OpInfo& op : *ops) {
                const bmi_site& st = op.d.site;
                if (st.kind != BMI_SITE_MASKSEMBLE) continue;
                for (auto& pr : h->perm)
                    if (pr.first == st.masks) {
                        const int width = op.d.kind == BMI_OP_HEAD ? h->tensors[op.d.in].c : op.cout;
                        const int rc = launch_mask_permute(st.masks, (float*)(p.ws + pr.second), st.num_masks, width, mask_cnt0, mask_stride,
                                                           p.stream);
                        if (rc != BMI_OK) return rc;
                        break;
                    }
            }
        p.permuted = true;
        p.mask_t_begin = t_begin;
        p.cnt0 = 0;
    }
    return forward_folded(h, p, t_begin, t_count);
}

int bmi_forward_mcd_exit(bmi_handle h, const float* x_nchw, int32_t batch, int32_t t_count, uint64_t seed, int32_t mask_cnt0,
                         double threshold, int32_t first_exit, double* S1, double* S2, double* SL, int32_t* exit_of_image,
                         int32_t* active_after, void* workspace, size_t workspace_bytes, bmi_stream stream) {
    if (!h || !x_nchw || !S1 || !S2 || !SL || !workspace || !exit_of_image || !active_after) return BMI_ERR_INVALID;
    BmiOptionScope opt_scope(&h->opts);
    if (batch < 1 || t_count < 1 || mask_cnt0 < 0 || first_exit < 0) return BMI_ERR_INVALID;
    if (h->max_batch == 0 || batch > h->max_batch) return BMI_ERR_INVALID;
    if (t_count > h->chunk || (h->f32 && !h->split)) return BMI_ERR_UNSUPPORTED;     // an exit's decision needs ALL samples of the stage in the workspace
    const int last = h->n_exits - 1;
    bool compacted = false;        // MASK / MAXPOOL / DENSE ops behind the first tested exit: not this entry point's contract
    for (const OpInfo& op : h->suffix) {
        if (compacted && (op.d.kind == BMI_OP_MASK || op.d.kind == BMI_OP_MAXPOOL || op.d.kind == BMI_OP_DENSE)) return BMI_ERR_UNSUPPORTED;
        compacted = compacted || (op.d.kind == BMI_OP_HEAD && op.d.out >= first_exit && op.d.out < last);
    }
    if (workspace_bytes < h->ws_bytes) return BMI_ERR_NOMEM;
    Pass p{x_nchw, (char*)workspace, (hipStream_t)stream, batch, seed, mask_cnt0};
    p.S1 = S1; p.S2 = S2; p.SL = SL;
    const hipStream_t s = p.stream;
    ActiveImages on(h, p.ws, batch, s);
    int rc = launch_fill_int(exit_of_image, batch, last, s);
    if (rc != BMI_OK) return rc;
    for (int x = 0; x < h->n_exits; ++x) active_after[x] = 0;
    for (const OpInfo& op : h->prefix) {
        rc = run_op(h, p, op, batch, 0);
        if (rc != BMI_OK) return rc;
    }
    for (const OpInfo& op : h->suffix) {
        rc = run_op(h, p, op, t_count * on.bc, 0, on.act, on.bc, on.rows);
        if (rc != BMI_OK) return rc;
        if (op.d.kind != BMI_OP_HEAD) continue;
        const int e = op.d.out;
        if (e < first_exit || e >= last) { active_after[e] = on.bc; continue; }
        // confidence test of exit e over the still-active images, on the device; the host only learns how many go on
        rc = launch_exit_decide(S1 + (size_t)e * batch * h->out_dim, h->out_dim, t_count, threshold, on.act, on.bc, on.next(), on.count_dev,
                                exit_of_image, e, s);
        if (rc != BMI_OK) return rc;
        int n_active = 0;
        rc = on.read_count(&n_active);
        if (rc != BMI_OK) return rc;
        active_after[e] = n_active;
        if (n_active == 0) return BMI_OK;                    // every image has left: the later stages do not run at all
        rc = on.take(n_active, t_count);
        if (rc != BMI_OK) return rc;
    }
    return BMI_OK;
}

// bmi_forward_mcd_exit_staged (ens null) and bmi_forward_mcd_exit_staged_ensemble: with ens every stage's heads also leave their logits in
// the one [t_count][E][batch][C] scratch (active images only), and ONE launch of ensemble.hip behind the last stage that ran adds, for
// every image, the exits it reached (n_e[b] = exit_of_image[b] + 1) to the ensemble sums; votes (bmi_forward_mcd_exit_staged_votes, with ens
// only): one launch of votes_rows.hip behind it, with the same n_e, adds their votes
static int exit_staged(bmi_handle h, const float* x_nchw, int32_t batch, int32_t t_count, uint64_t seed, int32_t mask_cnt0,
                       const bmi_exit_rule* rule, double* S1, double* S2, double* SL, double* SH, int32_t* exit_of_image, int32_t* active_after,
                       void* workspace, size_t workspace_bytes, bmi_stream stream, const EnsembleSums* ens, const VoteCounts* votes = nullptr) {
    if (!h || !x_nchw || !rule || !S1 || !S2 || !SL || !workspace || !exit_of_image || !active_after) return BMI_ERR_INVALID;
    BmiOptionScope opt_scope(&h->opts);
    if (rule->criterion != BMI_EXIT_CONFIDENCE && rule->criterion != BMI_EXIT_MARGIN) return BMI_ERR_INVALID;
    if ((rule->ensemble != 0 && rule->ensemble != 1) || rule->threshold != rule->threshold) return BMI_ERR_INVALID;
    if (rule->first_exit < 0 || rule->first_exit >= h->n_exits) return BMI_ERR_INVALID;
    if (batch < 1 || t_count < 1 || mask_cnt0 < 0) return BMI_ERR_INVALID;
    if (h->max_batch == 0 || batch > h->max_batch) return BMI_ERR_INVALID;
    if (t_count > h->chunk || (h->f32 && !h->split)) return BMI_ERR_UNSUPPORTED;     // a decision needs ALL samples of its stage in the workspace
    const int fe = rule->first_exit, last = h->n_exits - 1;
    for (const OpInfo& op : h->suffix)
        if (op.d.kind == OP_MASKBITS && op_stage(op, fe) > 0) return BMI_ERR_UNSUPPORTED;     // (its conv_igemm readers have no row-table form)
    if (!h->staged_ok[fe]) return BMI_ERR_UNSUPPORTED;
    if (workspace_bytes < h->ws_bytes) return BMI_ERR_NOMEM;
    Pass p{x_nchw, (char*)workspace, (hipStream_t)stream, batch, seed, mask_cnt0};
    p.S1 = S1; p.S2 = S2; p.SL = SL; p.SH = SH;
    if (ens) { p.logits = ens->scratch; p.logits_t_begin = 0; }
    const hipStream_t s = p.stream;
    ActiveImages on(h, p.ws, batch, s);
    int rc = launch_fill_int(exit_of_image, batch, last, s);
    if (rc != BMI_OK) return rc;
    for (int x = 0; x < h->n_exits; ++x) active_after[x] = 0;
    // the ensemble read-out behind the last stage that ran: exit_of_image is final and both image lists are dead (n_e takes the first)
    auto ensemble_readout = [&]() -> int {
        if (!ens) return BMI_OK;
        ProfScope prof(h, BMI_PROFILE_ENSEMBLE, s);
        prof.r.images = t_count * batch;
        int* const n_e = on.lists[0];
        const int rce = launch_exit_counts(exit_of_image, batch, n_e, s);
        if (rce != BMI_OK) return rce;
        const int rca = ensemble_add(h, *ens, t_count, batch, s, EnsRows{nullptr, 0, n_e});
        if (rca != BMI_OK || !votes) return rca;
        // (not recorded, as in forward_folded: the profile table has no slot for it)
        return launch_vote_counts_rows(ens->scratch, t_count, h->n_exits, batch, h->out_dim, h->cal, EnsRows{nullptr, 0, n_e}, votes->V,
                                       votes->nonfinite, s);
    };
    std::vector<const OpInfo*> stage_ops;
    for (int k = 0; fe + k <= last; ++k) {
        // the stage's prefix ops once per active image (rows = the active list); those without a row-table form over the whole batch
        for (const OpInfo& op : h->prefix) {
            if (op_stage(op, fe) != k) continue;
            rc = (on.act && prefix_row_form(h, op)) ? run_op(h, p, op, on.bc, 0, on.act, on.bc, on.act) : run_op(h, p, op, batch, 0);
            if (rc != BMI_OK) return rc;
        }
        stage_ops.clear();
        for (const OpInfo& op : h->suffix)
            if (op_stage(op, fe) == k) stage_ops.push_back(&op);
        rc = run_suffix_ops(h, p, stage_ops.size(), [&](size_t i) -> const OpInfo& { return *stage_ops[i]; }, t_count * on.bc, 0, on.act, on.bc, on.rows);
        if (rc != BMI_OK) return rc;
        const int e = fe + k;          // the exit tested after this stage (none after the last)
        for (const OpInfo* op : stage_ops)
            if (op->d.kind == BMI_OP_HEAD && (op->d.out != e || e == last)) active_after[op->d.out] = on.bc;
        if (e == last) break;
        rc = launch_exit_rule_decide(S1, batch, h->out_dim, t_count, rule->threshold, rule->criterion == BMI_EXIT_MARGIN, rule->ensemble, on.act, on.bc,
                                     on.next(), on.count_dev, exit_of_image, e, s, h->cal.ens_w, h->n_exits);
        if (rc != BMI_OK) return rc;
        int n_active = 0;
        rc = on.read_count(&n_active);
        if (rc != BMI_OK) return rc;
        active_after[e] = n_active;
        if (n_active == 0) return ensemble_readout();        // every image has left: the later stages do not run at all
        rc = on.take(n_active, t_count);
        if (rc != BMI_OK) return rc;
    }
    return ensemble_readout();
}

int bmi_forward_mcd_exit_staged(bmi_handle h, const float* x_nchw, int32_t batch, int32_t t_count, uint64_t seed, int32_t mask_cnt0,
                                const bmi_exit_rule* rule, double* S1, double* S2, double* SL, double* SH, int32_t* exit_of_image,
                                int32_t* active_after, void* workspace, size_t workspace_bytes, bmi_stream stream) {
    return exit_staged(h, x_nchw, batch, t_count, seed, mask_cnt0, rule, S1, S2, SL, SH, exit_of_image, active_after, workspace, workspace_bytes,
                       stream, nullptr);
}

int bmi_forward_mcd_exit_staged_ensemble(bmi_handle h, const float* x_nchw, int32_t batch, int32_t t_count, uint64_t seed, int32_t mask_cnt0,
                                         const bmi_exit_rule* rule, double* S1, double* S2, double* SL, double* SH, double* Q1, double* Q2,
                                         double* QH, void* scratch, size_t scratch_bytes, int32_t* exit_of_image, int32_t* active_after,
                                         void* workspace, size_t workspace_bytes, bmi_stream stream) {
    const int rce = ensemble_args_ok(h, batch, Q1, Q2, QH, scratch, scratch_bytes);
    if (rce != BMI_OK) return rce;
    const EnsembleSums ens{Q1, Q2, QH, (float*)scratch};
    return exit_staged(h, x_nchw, batch, t_count, seed, mask_cnt0, rule, S1, S2, SL, SH, exit_of_image, active_after, workspace, workspace_bytes,
                       stream, &ens);
}

int bmi_forward_mcd_exit_staged_votes(bmi_handle h, const float* x_nchw, int32_t batch, int32_t t_count, uint64_t seed, int32_t mask_cnt0,
                                      const bmi_exit_rule* rule, double* S1, double* S2, double* SL, double* SH, double* Q1, double* Q2,
                                      double* QH, int32_t* V, int32_t* nonfinite, void* scratch, size_t scratch_bytes, int32_t* exit_of_image,
                                      int32_t* active_after, void* workspace, size_t workspace_bytes, bmi_stream stream) {
    if (!V) return BMI_ERR_INVALID;
    const int rce = ensemble_args_ok(h, batch, Q1, Q2, QH, scratch, scratch_bytes);
    if (rce != BMI_OK) return rce;
    if (!vote_counts_takes(h->chunk, h->n_exits, batch, h->out_dim)) return BMI_ERR_UNSUPPORTED;
    const EnsembleSums ens{Q1, Q2, QH, (float*)scratch};
    const VoteCounts votes{V, nonfinite};
    return exit_staged(h, x_nchw, batch, t_count, seed, mask_cnt0, rule, S1, S2, SL, SH, exit_of_image, active_after, workspace, workspace_bytes,
                       stream, &ens, &votes);
}

// bmi_forward_mcd_adaptive (ens null) and bmi_forward_mcd_adaptive_ensemble: with ens every step's heads also leave their logits in the
// scratch (one step of [t_step][E][batch][C]) and one launch of ensemble.hip behind them adds the step's samples of the images that ran it
// to the ensemble sums — the full form while nobody has retired, the image-list form afterwards; stop_on = BMI_STOP_ON_ENSEMBLE: the rule
// reads Q1 / Q2 at row test_exit in place of S1 / S2.  votes (bmi_forward_mcd_adaptive_votes, with ens only): one launch of votes_rows.hip
// behind the ensemble launch adds the step's votes of the same images; rule BMI_STOP_VOTES then decides on row test_exit of V[stop_on],
// threshold = the slack.  rule_rc: the entry point's own verdict on rule and threshold (which rules it takes is its contract, not this
// function's), returned where the rule was always checked
static int adaptive(bmi_handle h, const float* x_nchw, int32_t batch, int32_t image_offset, int32_t t_max, int32_t t_step, uint64_t seed,
                    int32_t mask_cnt0, int32_t rule, double threshold, int32_t test_exit, double* S1, double* S2, double* SL, double* SH,
                    int32_t* t_used, uint8_t* converged, int32_t* active_after_step, void* workspace, size_t workspace_bytes, bmi_stream stream,
                    const EnsembleSums* ens, int stop_on, int rule_rc, const VoteCounts* votes = nullptr) {
    const int rco = bmi_image_offset_ok(h, image_offset);      // (a null handle: BMI_ERR_INVALID)
    if (rco != BMI_OK) return rco;
    BmiOptionScope opt_scope(&h->opts);
    if (!x_nchw || !S1 || !S2 || !SL || !t_used || !active_after_step || !workspace) return BMI_ERR_INVALID;
    if (batch < 1 || t_max < 1 || t_step < 1 || mask_cnt0 < 0) return BMI_ERR_INVALID;
    if (rule_rc != BMI_OK) return rule_rc;
    if (test_exit < 0 || test_exit >= h->n_exits) return BMI_ERR_INVALID;
    if (h->max_batch == 0 || batch > h->max_batch) return BMI_ERR_INVALID;
    if (t_step > h->chunk || (h->f32 && !h->split)) return BMI_ERR_UNSUPPORTED;     // (a step is one suffix chunk: the row table holds chunk x max_batch)
    for (const OpInfo& op : h->suffix)
        if (op.d.kind == OP_MASKBITS) return BMI_ERR_UNSUPPORTED;
    if (workspace_bytes < h->ws_bytes) return BMI_ERR_NOMEM;
    Pass p{x_nchw, (char*)workspace, (hipStream_t)stream, batch, seed, mask_cnt0};
    p.b0 = image_offset;
    p.S1 = S1; p.S2 = S2; p.SL = SL; p.SH = SH;
    const hipStream_t s = p.stream;
    ActiveImages on(h, p.ws, batch, s);      // act null: every image is still active — the step runs bmi_forward_mcd's kernels
    const size_t eo = (size_t)test_exit * batch * h->out_dim;
    const double* const R1 = (stop_on == BMI_STOP_ON_ENSEMBLE ? ens->Q1 : S1) + eo;      // the [batch][C] sums the rule reads
    const double* const R2 = (stop_on == BMI_STOP_ON_ENSEMBLE ? ens->Q2 : S2) + eo;
    const bool by_votes = rule == BMI_STOP_VOTES;      // (only with votes: rule_rc)
    // the [batch][C] counts the vote rule reads, and its slack
    const int* const RV = votes ? votes->V + ((size_t)(stop_on == BMI_STOP_ON_ENSEMBLE ? 1 : 0) * h->n_exits + test_exit) * batch * h->out_dim : nullptr;
    const int slack = by_votes ? (int)threshold : 0;
    const int n_steps = (t_max + t_step - 1) / t_step;
    for (int k = 0; k < n_steps; ++k) active_after_step[k] = 0;
    int rc;
    for (const OpInfo& op : h->prefix) {
        rc = run_op(h, p, op, batch, 0);
        if (rc != BMI_OK) return rc;
    }
    for (int k = 0, t0 = 0; k < n_steps; ++k, t0 += t_step) {
        const int tc = std::min(t_step, t_max - t0);
        if (ens) { p.logits = ens->scratch; p.logits_t_begin = t0; }
        rc = run_suffix(h, p, tc * on.bc, t0, on.act, on.bc, on.rows);
        if (rc != BMI_OK) return rc;
        if (ens) {
            ProfScope prof(h, BMI_PROFILE_ENSEMBLE, s);
            prof.r.images = tc * on.bc;
            rc = ensemble_add(h, *ens, tc, batch, s, EnsRows{on.act, on.bc, nullptr});
            if (rc != BMI_OK) return rc;
        }
        if (votes) {        // (not recorded, as in forward_folded: the profile table has no slot for it)
            rc = launch_vote_counts_rows(ens->scratch, tc, h->n_exits, batch, h->out_dim, h->cal, EnsRows{on.act, on.bc, nullptr}, votes->V,
                                         votes->nonfinite, s);
            if (rc != BMI_OK) return rc;
        }
        // the stop rule over the still-active images, on the device; the host only learns how many go on
        rc = by_votes ? launch_vote_decide(RV, batch, h->out_dim, t0 + tc, t_max, slack, on.act, on.bc, on.next(), on.count_dev, t_used, s)
                      : launch_adaptive_decide(R1, R2, h->out_dim, t0 + tc, rule, threshold, on.act, on.bc, on.next(), on.count_dev, t_used, s);
        if (rc != BMI_OK) return rc;
        int n_active = 0;
        rc = on.read_count(&n_active);
        if (rc != BMI_OK) return rc;
        active_after_step[k] = n_active;
        if (n_active == 0 || k + 1 == n_steps) break;
        if (n_active == batch) continue;           // nobody has retired yet: the next step runs on the full grids too
        rc = on.take(n_active, std::min(t_step, t_max - t0 - t_step));
        if (rc != BMI_OK) return rc;
    }
    if (!converged) return BMI_OK;
    return by_votes ? launch_vote_converged(RV, h->out_dim, t_max, slack, batch, t_used, converged, s)
                    : launch_adaptive_converged(R1, R2, h->out_dim, rule, threshold, batch, t_used, converged, s);
}

// BMI_STOP_SEM / BMI_STOP_MARGIN: the rules every adaptive entry point takes
static int moment_rule_rc(int32_t rule) { return rule == BMI_STOP_SEM || rule == BMI_STOP_MARGIN ? BMI_OK : BMI_ERR_INVALID; }

int bmi_forward_mcd_adaptive(bmi_handle h, const float* x_nchw, int32_t batch, int32_t image_offset, int32_t t_max,
                             int32_t t_step, uint64_t seed, int32_t mask_cnt0, int32_t rule, double threshold,
                             int32_t test_exit, double* S1, double* S2, double* SL, double* SH, int32_t* t_used,
                             uint8_t* converged, int32_t* active_after_step, void* workspace, size_t workspace_bytes,
                             bmi_stream stream) {
    return adaptive(h, x_nchw, batch, image_offset, t_max, t_step, seed, mask_cnt0, rule, threshold, test_exit, S1, S2, SL, SH, t_used, converged,
                    active_after_step, workspace, workspace_bytes, stream, nullptr, BMI_STOP_ON_EXIT, moment_rule_rc(rule));
}

int bmi_forward_mcd_adaptive_ensemble(bmi_handle h, const float* x_nchw, int32_t batch, int32_t image_offset, int32_t t_max, int32_t t_step,
                                      uint64_t seed, int32_t mask_cnt0, int32_t rule, double threshold, int32_t test_exit, int32_t stop_on,
                                      double* S1, double* S2, double* SL, double* SH, double* Q1, double* Q2, double* QH, void* scratch,
                                      size_t scratch_bytes, int32_t* t_used, uint8_t* converged, int32_t* active_after_step, void* workspace,
                                      size_t workspace_bytes, bmi_stream stream) {
    if (stop_on != BMI_STOP_ON_EXIT && stop_on != BMI_STOP_ON_ENSEMBLE) return BMI_ERR_INVALID;      // (BMI_ERR_INVALID like the null checks next)
    const int rce = ensemble_args_ok(h, batch, Q1, Q2, QH, scratch, scratch_bytes);
    if (rce != BMI_OK) return rce;
    const EnsembleSums ens{Q1, Q2, QH, (float*)scratch};
    return adaptive(h, x_nchw, batch, image_offset, t_max, t_step, seed, mask_cnt0, rule, threshold, test_exit, S1, S2, SL, SH, t_used, converged,
                    active_after_step, workspace, workspace_bytes, stream, &ens, stop_on, moment_rule_rc(rule));
}

int bmi_forward_mcd_adaptive_votes(bmi_handle h, const float* x_nchw, int32_t batch, int32_t image_offset, int32_t t_max, int32_t t_step,
                                   uint64_t seed, int32_t mask_cnt0, int32_t rule, double threshold, int32_t test_exit, int32_t stop_on,
                                   double* S1, double* S2, double* SL, double* SH, double* Q1, double* Q2, double* QH, int32_t* V,
                                   int32_t* nonfinite, void* scratch, size_t scratch_bytes, int32_t* t_used, uint8_t* converged,
                                   int32_t* active_after_step, void* workspace, size_t workspace_bytes, bmi_stream stream) {
    if (!V || (stop_on != BMI_STOP_ON_EXIT && stop_on != BMI_STOP_ON_ENSEMBLE)) return BMI_ERR_INVALID;
    const int rce = ensemble_args_ok(h, batch, Q1, Q2, QH, scratch, scratch_bytes);
    if (rce != BMI_OK) return rce;
    if (!vote_counts_takes(h->chunk, h->n_exits, batch, h->out_dim)) return BMI_ERR_UNSUPPORTED;
    // the vote rule's threshold is its slack: a whole number of samples (a NaN fails the first comparison)
    const bool slack_ok = threshold >= 0.0 && threshold <= (double)INT32_MAX && threshold == std::floor(threshold);
    const int rule_rc = rule == BMI_STOP_VOTES ? (slack_ok ? BMI_OK : BMI_ERR_INVALID) : moment_rule_rc(rule);
    const EnsembleSums ens{Q1, Q2, QH, (float*)scratch};
    const VoteCounts votes{V, nonfinite};
    return adaptive(h, x_nchw, batch, image_offset, t_max, t_step, seed, mask_cnt0, rule, threshold, test_exit, S1, S2, SL, SH, t_used, converged,
                    active_after_step, workspace, workspace_bytes, stream, &ens, stop_on, rule_rc, &votes);
}

int bmi_finalize_per_image(int32_t n_exits, int32_t batch, int32_t out_dim, const int32_t* t_used, const double* S1,
                           const double* S2, const double* SL, const double* SH, double* mean, double* var,
                           double* logit_mean, double* pred_entropy, double* exp_entropy, double* mutual_info,
                           int32_t* nonfinite, bmi_stream stream) {
    if (!t_used || !S1 || !S2 || !SL || !mean || !var || !logit_mean || n_exits < 1 || batch < 1 || out_dim < 1) return BMI_ERR_INVALID;
    const bool any_unc = SH || pred_entropy || exp_entropy || mutual_info;
    if (any_unc && !(SH && pred_entropy && exp_entropy && mutual_info)) return BMI_ERR_INVALID;
    if ((int64_t)n_exits * batch > INT32_MAX) return BMI_ERR_UNSUPPORTED;
    return launch_finalize_per_image(n_exits, batch, out_dim, t_used, S1, S2, SL, SH, mean, var, logit_mean, pred_entropy, exp_entropy,
                                     mutual_info, nonfinite, (hipStream_t)stream);
}

int bmi_finalize(int64_t n, int32_t t_total, const double* S1, const double* S2, const double* SL, double* mean,
                 double* var, double* logit_mean, bmi_stream stream) {
    if (!S1 || !S2 || !SL || !mean || !var || !logit_mean) return BMI_ERR_INVALID;
    return launch_finalize(n, t_total, S1, S2, SL, mean, var, logit_mean, nullptr, (hipStream_t)stream);
}

int bmi_finalize_checked(int64_t n, int32_t t_total, const double* S1, const double* S2, const double* SL, double* mean,
                         double* var, double* logit_mean, int32_t* nonfinite, bmi_stream stream) {
    if (!S1 || !S2 || !SL || !mean || !var || !logit_mean || !nonfinite) return BMI_ERR_INVALID;
    return launch_finalize(n, t_total, S1, S2, SL, mean, var, logit_mean, nonfinite, (hipStream_t)stream);
}

int bmi_finalize_uncertainty(int32_t n_exits, int32_t batch, int32_t out_dim, int32_t t_total, const double* S1, const double* SH,
                             double* pred_entropy, double* exp_entropy, double* mutual_info, int32_t* nonfinite, bmi_stream stream) {
    if (!S1 || !SH || !pred_entropy || !exp_entropy || !mutual_info || n_exits < 1 || batch < 1 || out_dim < 1 || t_total < 1)
        return BMI_ERR_INVALID;
    if ((int64_t)n_exits * batch > INT32_MAX) return BMI_ERR_UNSUPPORTED;
    return launch_finalize_uncertainty(n_exits * batch, out_dim, t_total, S1, SH, pred_entropy, exp_entropy, mutual_info, nonfinite,
                                       (hipStream_t)stream);
}

int bmi_finalize_ensemble(int32_t n_exits, int32_t batch, int32_t out_dim, int32_t t_total, const double* Q1, const double* Q2, const double* QH,
                          double* ens_mean, double* ens_var, double* pred_entropy, double* exp_entropy, double* mutual_info, int32_t* nonfinite,
                          bmi_stream stream) {
    if (!Q1 || !Q2 || !QH || !ens_mean || !ens_var || !pred_entropy || !exp_entropy || !mutual_info || n_exits < 1 || batch < 1 || out_dim < 1 ||
        t_total < 1)
        return BMI_ERR_INVALID;
    if ((int64_t)n_exits * batch > INT32_MAX) return BMI_ERR_UNSUPPORTED;
    return launch_finalize_ensemble(n_exits * batch, out_dim, t_total, Q1, Q2, QH, ens_mean, ens_var, pred_entropy, exp_entropy, mutual_info,
                                    nonfinite, (hipStream_t)stream);
}

int bmi_finalize_ensemble_per_image(int32_t n_exits, int32_t batch, int32_t out_dim, const int32_t* t_used, const double* Q1, const double* Q2,
                                    const double* QH, double* ens_mean, double* ens_var, double* pred_entropy, double* exp_entropy,
                                    double* mutual_info, int32_t* nonfinite, bmi_stream stream) {
    if (!t_used || !Q1 || !Q2 || !QH || !ens_mean || !ens_var || !pred_entropy || !exp_entropy || !mutual_info || n_exits < 1 || batch < 1 ||
        out_dim < 1)
        return BMI_ERR_INVALID;
    if ((int64_t)n_exits * batch > INT32_MAX) return BMI_ERR_UNSUPPORTED;
    return launch_finalize_ensemble_per_image(n_exits, batch, out_dim, t_used, Q1, Q2, QH, ens_mean, ens_var, pred_entropy, exp_entropy,
                                              mutual_info, nonfinite, (hipStream_t)stream);
}

// bmi_ensemble_moments, _weighted, _vector and _matrix: cal holds what the entry point was given beside tau (the weights, the vector scaling)
static int ensemble_moments_entry(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const float* tau, Calibration cal, double* Q1,
                                  double* Q2, double* QH, bmi_stream stream) {
    if (!logits || !Q1 || !Q2 || !QH || T < 1 || E < 1 || B < 1 || C < 1) return BMI_ERR_INVALID;
    if (!ensemble_takes(E, C)) return BMI_ERR_UNSUPPORTED;
    if (tau && !cal.set_tau(tau, E)) return BMI_ERR_INVALID;
    return launch_ensemble_moments(logits, T, E, B, C, cal, EnsRows(), Q1, Q2, QH, (hipStream_t)stream);
}

int bmi_ensemble_moments(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const float* tau, double* Q1, double* Q2, double* QH,
                         bmi_stream stream) {
    return ensemble_moments_entry(logits, T, E, B, C, tau, Calibration(), Q1, Q2, QH, stream);
}

int bmi_ensemble_moments_weighted(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const float* tau, const double* W_device,
                                  double* Q1, double* Q2, double* QH, bmi_stream stream) {
    if (!W_device) return BMI_ERR_INVALID;
    Calibration cal;
    cal.ens_w = W_device;
    return ensemble_moments_entry(logits, T, E, B, C, tau, cal, Q1, Q2, QH, stream);
}

int bmi_ensemble_moments_vector(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const float* scale_device, const float* bias_device,
                                const double* W_device, double* Q1, double* Q2, double* QH, bmi_stream stream) {
    if (!scale_device || !bias_device) return BMI_ERR_INVALID;
    Calibration cal;
    cal.vec_scale = scale_device; cal.vec_bias = bias_device; cal.ens_w = W_device;
    return ensemble_moments_entry(logits, T, E, B, C, nullptr, cal, Q1, Q2, QH, stream);
}

int bmi_ensemble_moments_matrix(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const float* matrix_device, const float* bias_device,
                                const double* W_device, double* Q1, double* Q2, double* QH, bmi_stream stream) {
    if (!matrix_device || !bias_device) return BMI_ERR_INVALID;
    Calibration cal;
    cal.mat = matrix_device; cal.mat_bias = bias_device; cal.ens_w = W_device;
    return ensemble_moments_entry(logits, T, E, B, C, nullptr, cal, Q1, Q2, QH, stream);
}

int bmi_vote_counts(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const float* tau, const float* scale_device,
                    const float* bias_device, const float* matrix_device, const double* W_device, int32_t* V, int32_t* nonfinite, bmi_stream stream) {
    if (!logits || !V || T < 1 || E < 1 || B < 1 || C < 1) return BMI_ERR_INVALID;
    Calibration cal;
    cal.vec_scale = scale_device;
    cal.mat = matrix_device;
    (matrix_device ? cal.mat_bias : cal.vec_bias) = bias_device;       // the bias belongs to the map that is given: alone, it fails check()
    cal.ens_w = W_device;
    if (tau) cal.inv_tau.assign(1, 1.f);                               // "a temperature is given", for check(); set_tau below replaces it
    if (cal.check() != BMI_OK) return BMI_ERR_INVALID;
    if (!vote_counts_takes(T, E, B, C)) return BMI_ERR_UNSUPPORTED;    // (E <= 32 before E entries of tau are read)
    if (tau && !cal.set_tau(tau, E)) return BMI_ERR_INVALID;
    return launch_vote_counts(logits, T, E, B, C, cal, V, nonfinite, (hipStream_t)stream);
}

int bmi_vote_counts_rows(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const float* tau, const float* scale_device,
                         const float* bias_device, const float* matrix_device, const double* W_device, const int32_t* list, int32_t list_count,
                         const int32_t* n_e, int32_t* V, int32_t* nonfinite, bmi_stream stream) {
    if (!logits || !V || T < 1 || E < 1 || B < 1 || C < 1) return BMI_ERR_INVALID;
    if (list && (list_count < 1 || list_count > B)) return BMI_ERR_INVALID;
    Calibration cal;
    cal.vec_scale = scale_device;
    cal.mat = matrix_device;
    (matrix_device ? cal.mat_bias : cal.vec_bias) = bias_device;       // (as in bmi_vote_counts)
    cal.ens_w = W_device;
    if (tau) cal.inv_tau.assign(1, 1.f);
    if (cal.check() != BMI_OK) return BMI_ERR_INVALID;
    if (!vote_counts_takes(T, E, B, C)) return BMI_ERR_UNSUPPORTED;
    if (tau && !cal.set_tau(tau, E)) return BMI_ERR_INVALID;
    return launch_vote_counts_rows(logits, T, E, B, C, cal, EnsRows{list, list ? list_count : 0, n_e}, V, nonfinite, (hipStream_t)stream);
}

int bmi_vote_decide(const int32_t* V, int32_t E, int32_t B, int32_t C, int32_t kind, int32_t test_exit, int32_t t, int32_t t_max, int32_t slack,
                    const int32_t* in_list, int32_t in_count, int32_t* out_list, int32_t* count, int32_t* t_used, bmi_stream stream) {
    if (!V || !out_list || !count || !t_used || E < 1 || B < 1 || C < 1) return BMI_ERR_INVALID;
    if (kind < 0 || kind > 1 || test_exit < 0 || test_exit >= E || t < 1 || t_max < t || slack < 0) return BMI_ERR_INVALID;
    if (in_count < 1 || in_count > B || in_list == out_list) return BMI_ERR_INVALID;
    return launch_vote_decide(V + ((size_t)kind * E + test_exit) * B * C, B, C, t, t_max, slack, in_list, in_count, out_list, count, t_used,
                              (hipStream_t)stream);
}

int bmi_finalize_votes(int32_t n_exits, int32_t batch, int32_t out_dim, const int32_t* V, int32_t* vote_class, double* variation_ratio,
                       double* vote_entropy, bmi_stream stream) {
    if (!V || !vote_class || !variation_ratio || !vote_entropy || n_exits < 1 || batch < 1 || out_dim < 1) return BMI_ERR_INVALID;
    if ((int64_t)2 * n_exits * batch > INT32_MAX / 64) return BMI_ERR_UNSUPPORTED;
    return launch_finalize_votes(2 * n_exits * batch, out_dim, V, vote_class, variation_ratio, vote_entropy, (hipStream_t)stream);
}

size_t bmi_nll_matrix_scratch_bytes(int32_t E, int32_t B, int32_t C) {
    if (E < 1 || B < 1 || C < 1) return 0;
    return (size_t)E * B * ((size_t)C * C + (size_t)C + 1) * sizeof(double);
}

int bmi_nll_matrix_scaling_grad(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const int32_t* labels, const double* matrix,
                                const double* bias, double* nll, double* grad_matrix, double* grad_bias, void* scratch, size_t scratch_bytes,
                                bmi_stream stream) {
    if (!logits || !labels || !matrix || !bias || !nll || !grad_matrix || !grad_bias || !scratch || T < 1 || E < 1 || B < 1 || C < 1)
        return BMI_ERR_INVALID;
    if (!nll_matrix_takes(E, B, C)) return BMI_ERR_UNSUPPORTED;
    if (scratch_bytes < bmi_nll_matrix_scratch_bytes(E, B, C)) return BMI_ERR_NOMEM;
    return launch_nll_matrix_scaling_grad(logits, T, E, B, C, labels, matrix, bias, nll, grad_matrix, grad_bias, (double*)scratch, (hipStream_t)stream);
}

size_t bmi_nll_vector_scratch_bytes(int32_t E, int32_t B, int32_t C) {
    if (E < 1 || B < 1 || C < 1) return 0;
    return (size_t)E * B * (2 * (size_t)C + 1) * sizeof(double);
}

int bmi_nll_vector_scaling_grad(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const int32_t* labels, const double* scale,
                                const double* bias, double* nll, double* grad_scale, double* grad_bias, void* scratch, size_t scratch_bytes,
                                bmi_stream stream) {
    if (!logits || !labels || !scale || !bias || !nll || !grad_scale || !grad_bias || !scratch || T < 1 || E < 1 || B < 1 || C < 1)
        return BMI_ERR_INVALID;
    if (!nll_vector_takes(E, B, C)) return BMI_ERR_UNSUPPORTED;
    if (scratch_bytes < bmi_nll_vector_scratch_bytes(E, B, C)) return BMI_ERR_NOMEM;
    return launch_nll_vector_scaling_grad(logits, T, E, B, C, labels, scale, bias, nll, grad_scale, grad_bias, (double*)scratch, (hipStream_t)stream);
}

size_t bmi_nll_temperature_scratch_bytes(int32_t E, int32_t B, int32_t G) {
    if (E < 1 || B < 1 || G < 1) return 0;
    return (size_t)E * G * B * sizeof(double);
}

int bmi_nll_temperature_grid(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const int32_t* labels, const float* tau_grid,
                             int32_t G, double* nll, void* scratch, size_t scratch_bytes, bmi_stream stream) {
    if (!logits || !labels || !tau_grid || !nll || !scratch || T < 1 || E < 1 || B < 1 || C < 1 || G < 1) return BMI_ERR_INVALID;
    if (scratch_bytes < bmi_nll_temperature_scratch_bytes(E, B, G)) return BMI_ERR_NOMEM;
    return launch_nll_temperature_grid(logits, T, E, B, C, labels, tau_grid, G, nll, (double*)scratch, (hipStream_t)stream);
}

size_t bmi_nll_ensemble_temperature_scratch_bytes(int32_t E, int32_t B, int32_t G) { return bmi_nll_temperature_scratch_bytes(E, B, G); }

int bmi_nll_ensemble_temperature_grid(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const int32_t* labels, const float* tau,
                                      uint32_t vary_mask, const float* tau_cand, int32_t G, double* nll, void* scratch, size_t scratch_bytes,
                                      bmi_stream stream) {
    if (!logits || !labels || !tau || !tau_cand || !nll || !scratch || T < 1 || E < 1 || B < 1 || C < 1 || G < 1) return BMI_ERR_INVALID;
    if (E < 32 && (vary_mask >> E) != 0) return BMI_ERR_INVALID;
    if (E > 32) return BMI_ERR_UNSUPPORTED;
    if (scratch_bytes < bmi_nll_ensemble_temperature_scratch_bytes(E, B, G)) return BMI_ERR_NOMEM;
    return launch_nll_ensemble_temperature_grid(logits, T, E, B, C, labels, tau, vary_mask, tau_cand, G, nll, (double*)scratch, (hipStream_t)stream);
}

size_t bmi_pass_accuracy_scratch_bytes(int32_t T, int32_t E, int32_t B) {
    if (T < 1 || E < 1 || B < 1) return 0;
    const unsigned __int128 bytes = (unsigned __int128)T * E * B * (sizeof(double) + 2 * sizeof(int32_t));
    return bytes > SIZE_MAX ? SIZE_MAX : (size_t)bytes;
}

int bmi_pass_accuracy(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const int32_t* labels, const int32_t* tops, int32_t K,
                      int32_t* hits, double* maxprob, int32_t* nonfinite, void* scratch, size_t scratch_bytes, bmi_stream stream) {
    if (!logits || !labels || !tops || !hits || !maxprob || !scratch || T < 1 || E < 1 || B < 1 || C < 1 || K < 1) return BMI_ERR_INVALID;
    if (!pass_accuracy_takes(T, E, B, C, K)) return BMI_ERR_UNSUPPORTED;
    for (int i = 0; i < K; ++i)
        if (tops[i] < 1) return BMI_ERR_INVALID;
    if (scratch_bytes < bmi_pass_accuracy_scratch_bytes(T, E, B)) return BMI_ERR_NOMEM;
    return launch_pass_accuracy(logits, T, E, B, C, labels, tops, K, hits, maxprob, nonfinite, scratch, (hipStream_t)stream);
}

int bmi_reliability_record(const double* mean, int32_t E, int32_t B, int32_t C, const int32_t* labels, int32_t n0, int32_t N_cap, uint32_t* keys,
                           uint8_t* hit, double* nll, double* brier, int32_t* counters, bmi_stream stream) {
    if (!mean || !labels || !keys || !hit || !nll || !brier || E < 1 || B < 1 || C < 1 || N_cap < 1 || n0 < 0 || (int64_t)n0 + B > N_cap)
        return BMI_ERR_INVALID;
    if (!reliability_record_takes(E, B, C)) return BMI_ERR_UNSUPPORTED;
    return launch_reliability_record(mean, E, B, C, labels, n0, N_cap, keys, hit, nll, brier, counters, (hipStream_t)stream);
}

size_t bmi_reliability_scratch_bytes(int32_t R, int32_t N, int32_t n_bins) { return reliability_scratch_bytes(R, N, n_bins); }

int bmi_reliability_table(const uint32_t* keys, const uint8_t* hit, const double* nll, const double* brier, int32_t R, int32_t N, int32_t N_cap,
                          int32_t n_bins, const float* edges_in, float* edges_out, int64_t* count, int64_t* hits, int64_t* conf_fix, double* sums,
                          void* scratch, size_t scratch_bytes, bmi_stream stream) {
    if (!keys || !hit || !nll || !brier || !edges_out || !count || !hits || !conf_fix || !sums || !scratch || R < 1 || N < 1 || N > N_cap ||
        n_bins < 1 || n_bins > BMI_REL_MAX_BINS)
        return BMI_ERR_INVALID;
    if (edges_in)
        for (int i = 0; i <= n_bins; ++i)
            if (!std::isfinite(edges_in[i]) || (i && edges_in[i] < edges_in[i - 1])) return BMI_ERR_INVALID;
    if (!reliability_table_takes(R, N, n_bins)) return BMI_ERR_UNSUPPORTED;
    if (scratch_bytes < bmi_reliability_scratch_bytes(R, N, n_bins)) return BMI_ERR_NOMEM;
    return launch_reliability_table(keys, hit, nll, brier, R, N, N_cap, n_bins, edges_in, edges_out, (long long*)count, (long long*)hits,
                                    (long long*)conf_fix, sums, scratch, (hipStream_t)stream);
}

int bmi_reliability_kde(const uint32_t* keys, const uint8_t* hit, int32_t R, int32_t N, int32_t N_cap, int32_t G, int32_t order, double bw_scale,
                        double* ece_kde, double* bw, double* sd, int64_t* n_data, int64_t* n_hit, int32_t* degenerate, double* density,
                        bmi_stream stream) {
    if (!keys || !hit || !ece_kde || !bw || !sd || !n_data || !n_hit || !degenerate || !density || R < 1 || N < 1 || N > N_cap ||
        G < BMI_KDE_MIN_GRID || G > BMI_KDE_MAX_GRID || (order != 1 && order != 2) || !std::isfinite(bw_scale) || !(bw_scale > 0.0))
        return BMI_ERR_INVALID;
    if (!reliability_kde_takes(R, N, G, bw_scale)) return BMI_ERR_UNSUPPORTED;
    return launch_reliability_kde(keys, hit, R, N, N_cap, G, order, bw_scale, ece_kde, bw, sd, (long long*)n_data, (long long*)n_hit, degenerate,
                                  density, (hipStream_t)stream);
}

int bmi_classwise_record(const double* mean, int32_t E, int32_t B, int32_t C, const int32_t* labels, int32_t n0, int32_t N_cap, uint32_t* pkeys,
                         int32_t* labels_rec, int32_t* counters, bmi_stream stream) {
    if (!mean || !labels || !pkeys || !labels_rec || E < 1 || B < 1 || C < 1 || N_cap < 1 || n0 < 0 || (int64_t)n0 + B > N_cap)
        return BMI_ERR_INVALID;
    if (!reliability_record_takes(E, B, C)) return BMI_ERR_UNSUPPORTED;
    return launch_classwise_record(mean, E, B, C, labels, n0, N_cap, pkeys, labels_rec, counters, (hipStream_t)stream);
}

int bmi_classwise_table(const uint32_t* pkeys, const int32_t* labels_rec, int32_t R, int32_t C, int32_t N, int32_t N_cap, int32_t n_bins,
                        const float* edges_in, float* edges_out, int64_t* count, int64_t* hits, int64_t* conf_fix, int64_t* valid,
                        bmi_stream stream) {
    if (!pkeys || !labels_rec || !edges_out || !count || !hits || !conf_fix || !valid || R < 1 || C < 1 || N < 1 || N > N_cap || n_bins < 1 ||
        n_bins > BMI_REL_MAX_BINS)
        return BMI_ERR_INVALID;
    if (edges_in)
        for (int i = 0; i <= n_bins; ++i)
            if (!std::isfinite(edges_in[i]) || (i && edges_in[i] < edges_in[i - 1])) return BMI_ERR_INVALID;
    if (!classwise_table_takes(R, C, N, n_bins)) return BMI_ERR_UNSUPPORTED;
    return launch_classwise_table(pkeys, labels_rec, R, C, N, N_cap, n_bins, edges_in, edges_out, (long long*)count, (long long*)hits,
                                  (long long*)conf_fix, (long long*)valid, (hipStream_t)stream);
}

int bmi_score_record(const double* score, int32_t R, int32_t B, int32_t direction, const uint32_t* valid_keys, int32_t n0, int32_t N_cap,
                     uint32_t* ukeys, int32_t* counter, bmi_stream stream) {
    if (!score || !ukeys || R < 1 || B < 1 || N_cap < 1 || n0 < 0 || (int64_t)n0 + B > N_cap || (direction != 1 && direction != -1))
        return BMI_ERR_INVALID;
    if (!score_record_takes(R, B)) return BMI_ERR_UNSUPPORTED;
    return launch_score_record(score, R, B, direction, valid_keys, n0, N_cap, ukeys, counter, (hipStream_t)stream);
}

size_t bmi_rank_scratch_bytes(int32_t R, int32_t N) { return rank_scratch_bytes(R, N); }

int bmi_rank_quality(const uint32_t* ukeys, const uint8_t* positive, int32_t R, int32_t N, int32_t N_cap, int32_t* rank, uint32_t* sorted_keys,
                     int32_t* curve, int64_t* counts, double* aurc_sum, void* scratch, size_t scratch_bytes, bmi_stream stream) {
    if (!ukeys || !positive || !rank || !sorted_keys || !curve || !counts || !aurc_sum || !scratch || R < 1 || N < 1 || N > N_cap)
        return BMI_ERR_INVALID;
    if (!rank_quality_takes(R, N)) return BMI_ERR_UNSUPPORTED;
    if (scratch_bytes < bmi_rank_scratch_bytes(R, N)) return BMI_ERR_NOMEM;
    return launch_rank_quality(ukeys, positive, R, N, N_cap, rank, sorted_keys, curve, (long long*)counts, aurc_sum, scratch, (hipStream_t)stream);
}

int bmi_exit_stat_record(const double* S1, int32_t E, int32_t B, int32_t C, int32_t t_count, int32_t criterion, const double* weights, int32_t n0,
                         int32_t N_cap, double* stat, bmi_stream stream) {
    if (!S1 || !stat || E < 1 || B < 1 || C < 1 || t_count < 1 || N_cap < 1 || n0 < 0 || (int64_t)n0 + B > N_cap ||
        (criterion != BMI_EXIT_CONFIDENCE && criterion != BMI_EXIT_MARGIN))
        return BMI_ERR_INVALID;
    if (!exit_stat_record_takes(E, B, C)) return BMI_ERR_UNSUPPORTED;
    return launch_exit_stat_record(S1, E, B, C, t_count, criterion == BMI_EXIT_MARGIN, weights, n0, N_cap, stat, (hipStream_t)stream);
}

size_t bmi_exit_policy_scratch_bytes(int32_t E, int32_t N, int32_t G) { return exit_policy_scratch_bytes(E, N, G); }

int bmi_exit_policy_sweep(const double* stat, int32_t E, int32_t N, int32_t N_cap, int32_t first_exit, const double* thresholds, int32_t G,
                          const uint32_t* keys, const uint8_t* hit, const double* nll, const double* brier, int64_t* count, int64_t* hits,
                          int64_t* invalid, uint8_t* exit_of, uint32_t* sel_keys, uint8_t* sel_hit, double* sel_nll, double* sel_brier,
                          void* scratch, size_t scratch_bytes, bmi_stream stream) {
    const int n_sel = (sel_keys != nullptr) + (sel_hit != nullptr) + (sel_nll != nullptr) + (sel_brier != nullptr);
    if (!stat || !thresholds || !keys || !hit || !nll || !brier || !count || !hits || !invalid || !scratch || (n_sel != 0 && n_sel != 4) ||
        E < 1 || N < 1 || G < 1 || N > N_cap || first_exit < 0 || first_exit >= E)
        return BMI_ERR_INVALID;
    if (!exit_policy_takes(E, N, G, n_sel == 4)) return BMI_ERR_UNSUPPORTED;
    if (scratch_bytes < bmi_exit_policy_scratch_bytes(E, N, G)) return BMI_ERR_NOMEM;
    return launch_exit_policy_sweep(stat, E, N, N_cap, first_exit, thresholds, G, keys, hit, nll, brier, (long long*)count, (long long*)hits,
                                    (long long*)invalid, exit_of, sel_keys, sel_hit, sel_nll, sel_brier, scratch, (hipStream_t)stream);
}

int bmi_profile_enable(bmi_handle h, int32_t enable) {
    if (!h) return BMI_ERR_INVALID;
    h->profiling = enable != 0;
    return BMI_OK;
}

int bmi_profile_read(bmi_handle h, double ms[BMI_PROFILE_SLOTS], int64_t launches[BMI_PROFILE_SLOTS]) {
    if (!h || !ms || !launches) return BMI_ERR_INVALID;
    for (int i = 0; i < BMI_PROFILE_SLOTS; ++i) { ms[i] = 0; launches[i] = 0; }
    for (int i = 0; i < BMI_CONV_FAMILIES; ++i) { h->fam_ms[i] = 0; h->fam_flops[i] = 0; h->fam_bytes[i] = 0; h->fam_launches[i] = 0; }
    int rc = BMI_OK;
    h->last.clear();
    for (auto& r : h->recs) {
        float t = 0.f;
        if (hipEventSynchronize(r.b) != hipSuccess || hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) rc = BMI_ERR_HIP;
        r.ms = t;
        h->last.push_back(r);
        if (r.slot >= 0 && r.slot < BMI_PROFILE_SLOTS) { ms[r.slot] += t; launches[r.slot] += 1; }
        if (r.slot == BMI_OP_CONV && r.family >= 0 && r.family < BMI_CONV_FAMILIES) {
            h->fam_ms[r.family] += t; h->fam_flops[r.family] += r.flops; h->fam_bytes[r.family] += r.bytes; h->fam_launches[r.family] += 1;
        }
        h->pool.push_back(r.a);
        h->pool.push_back(r.b);
    }
    h->recs.clear();
    return rc;
}

int bmi_profile_conv_families(bmi_handle h, double ms[BMI_CONV_FAMILIES], int64_t launches[BMI_CONV_FAMILIES],
                              double flops[BMI_CONV_FAMILIES], double bytes[BMI_CONV_FAMILIES]) {
    if (!h || !ms || !launches || !flops || !bytes) return BMI_ERR_INVALID;
    for (int i = 0; i < BMI_CONV_FAMILIES; ++i) { ms[i] = h->fam_ms[i]; launches[i] = h->fam_launches[i]; flops[i] = h->fam_flops[i]; bytes[i] = h->fam_bytes[i]; }
    return BMI_OK;
}

int bmi_profile_launches(bmi_handle h, int32_t capacity, int32_t* count, int32_t* kind, int32_t* family, int32_t* out_tensor,
                         int32_t* images, double* ms, double* flops, double* bytes) {
    if (!h || !count || capacity < 0) return BMI_ERR_INVALID;
    *count = (int32_t)h->last.size();
    for (int i = 0; i < *count && i < capacity; ++i) {
        const ProfRec& r = h->last[i];
        if (kind) kind[i] = r.slot;
        if (family) family[i] = r.family;
        if (out_tensor) out_tensor[i] = r.out;
        if (images) images[i] = r.images;
        if (ms) ms[i] = r.ms;
        if (flops) flops[i] = r.flops;
        if (bytes) bytes[i] = r.bytes;
    }
    return BMI_OK;
}

// ---- single-kernel entry points -------------------------------------------------------------

int bmi_philox_mask(uint8_t* keep, int64_t n, uint64_t seed, int32_t site, int32_t t, float p, bmi_stream stream) {
    if (!keep) return BMI_ERR_INVALID;
    return launch_philox_mask(keep, n, seed, site, t, p, (hipStream_t)stream);
}

int bmi_stem_conv_fwd(const float* x_nchw, const float* weight, const float* scale, const float* bias, void* out_nhwc,
                      int32_t n, int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t ksize, int32_t stride,
                      int32_t pad, int32_t relu, bmi_stream stream) {
    if (!x_nchw || !weight || !out_nhwc) return BMI_ERR_INVALID;
    return launch_stem_conv(x_nchw, weight, scale, bias, (_Float16*)out_nhwc, n, cin, h, w, cout, ksize, stride, pad, relu,
                            opt_unit_dtype(), (hipStream_t)stream);
}

int bmi_mask_bits(void* bits, int32_t n, int32_t hw, int32_t c, const bmi_site* site, int32_t batch, int32_t t0,
                  uint64_t seed, bmi_stream stream) {
    if (!bits || !site || !site_ok(*site)) return BMI_ERR_INVALID;
    return launch_mask_bits((uint8_t*)bits, n, hw, c, resolve_site(site, seed, 0), batch, t0, (hipStream_t)stream);
}

int bmi_conv_igemm_fwd(const void* in, const void* in_keep_bits, float out_mul, const void* weight,
                       const float* scale, const float* bias, const void* res, void* out,
                       int32_t n, int32_t in_mod, int32_t res_mod, int32_t h, int32_t w, int32_t cin, int32_t cout,
                       int32_t ksize, int32_t stride, int32_t pad, int32_t relu, const bmi_site* site,
                       int32_t batch, int32_t t0, uint64_t seed, int32_t mask_cnt0, bmi_stream stream) {
    if (!in || !weight || !out || ksize < 1 || stride < 1 || pad < 0) return BMI_ERR_INVALID;
    if (site && !site_ok(*site)) return BMI_ERR_INVALID;
    ConvArgs a;
    std::memset(&a, 0, sizeof(a));
    a.bf16 = opt_unit_dtype() == BMI_DTYPE_BF16;
    a.in = (const _Float16*)in; a.wgt = (const _Float16*)weight; a.scale = scale; a.bias = bias;
    a.res = (const _Float16*)res; a.out = (_Float16*)out;
    a.N = n; a.in_mod = in_mod; a.res_mod = res_mod;
    a.H = h; a.W = w; a.Cin = cin; a.Cout = cout;
    a.Ho = (h + 2 * pad - ksize) / stride + 1;
    a.Wo = (w + 2 * pad - ksize) / stride + 1;
    a.ksize = ksize; a.stride = stride; a.pad = pad; a.relu = relu;
    a.M = n * a.Ho * a.Wo;
    a.B = batch; a.t0 = t0;
    a.site = resolve_site(site, seed, mask_cnt0);
    a.in_bits = (const uint8_t*)in_keep_bits;
    a.out_mul = out_mul;
    if (opt_unit_dtype() == BMI_DTYPE_F32) return launch_conv_exact(a, (hipStream_t)stream);
    if (unit_f32act()) return launch_conv_split(a, opt_unit_dtype() == BMI_DTYPE_BF16X3, (hipStream_t)stream);
    return launch_conv(a, (hipStream_t)stream);
}

int bmi_conv1x1_seam_fwd(const void* in, const void* weight3, const float* scale3, const float* bias3, const void* res, void* out_wide,
                         const void* weight1, const float* scale1, const float* bias1, void* out_narrow, int32_t n, int32_t h, int32_t w,
                         int32_t cmid, int32_t cw, int32_t cn, int32_t relu1, bmi_stream stream) {
    if (!in || !weight3 || !res || !out_wide || !weight1 || !out_narrow || n <= 0) return BMI_ERR_INVALID;
    if (opt_unit_dtype() != BMI_DTYPE_F16 && opt_unit_dtype() != BMI_DTYPE_BF16) return BMI_ERR_UNSUPPORTED;
    ConvArgs a, b;
    std::memset(&a, 0, sizeof(a));
    a.bf16 = opt_unit_dtype() == BMI_DTYPE_BF16;
    a.in = (const _Float16*)in; a.wgt = (const _Float16*)weight3; a.scale = scale3; a.bias = bias3;
    a.res = (const _Float16*)res; a.out = (_Float16*)out_wide;
    a.N = n; a.in_mod = n; a.res_mod = n;
    a.H = a.Ho = h; a.W = a.Wo = w; a.Cin = cmid; a.Cout = cw;
    a.ksize = 1; a.stride = 1; a.pad = 0; a.relu = 1;
    a.M = n * h * w; a.B = n; a.out_mul = 1.f;
    a.site = resolve_site(nullptr, 0, 0);
    b = a;
    b.in = a.out; b.wgt = (const _Float16*)weight1; b.scale = scale1; b.bias = bias1; b.res = nullptr; b.res_mod = 0;
    b.out = (_Float16*)out_narrow; b.Cin = cw; b.Cout = cn; b.relu = relu1;
    const int rc = launch_conv1x1_seam(a, b, (hipStream_t)stream);
    if (rc != BMI_ERR_UNSUPPORTED) return rc;
    const int rc1 = launch_conv(a, (hipStream_t)stream);      // the engine's fallback: the two launches
    return rc1 != BMI_OK ? rc1 : launch_conv(b, (hipStream_t)stream);
}

int bmi_conv_pair_fwd(const void* in, const void* weight_a, const float* scale_a, const float* bias_a, void* out_a,
                      const void* weight_b, const float* scale_b, const float* bias_b, void* out_b, int32_t n,
                      int32_t in_mod, int32_t h, int32_t w, int32_t cin, int32_t cout_a, int32_t cout_b, int32_t ksize,
                      int32_t stride, int32_t pad, int32_t relu, bmi_stream stream) {
    if (!in || !weight_a || !weight_b || !out_a || !out_b || ksize < 1 || stride < 1 || pad < 0) return BMI_ERR_INVALID;
    ConvArgs a;
    std::memset(&a, 0, sizeof(a));
    a.bf16 = opt_unit_dtype() == BMI_DTYPE_BF16;
    a.in = (const _Float16*)in; a.wgt = (const _Float16*)weight_a; a.scale = scale_a; a.bias = bias_a; a.out = (_Float16*)out_a;
    a.wgt_b = (const _Float16*)weight_b; a.scale_b = scale_b; a.bias_b = bias_b; a.out_b = (_Float16*)out_b;
    a.split = cout_a;
    a.N = n; a.in_mod = in_mod; a.H = h; a.W = w; a.Cin = cin; a.Cout = cout_a + cout_b;
    a.Ho = (h + 2 * pad - ksize) / stride + 1;
    a.Wo = (w + 2 * pad - ksize) / stride + 1;
    a.ksize = ksize; a.stride = stride; a.pad = pad; a.relu = relu;
    a.M = n * a.Ho * a.Wo;
    a.B = n; a.out_mul = 1.f;
    a.site = resolve_site(nullptr, 0, 0);
    if (opt_unit_dtype() == BMI_DTYPE_F32) return BMI_ERR_UNSUPPORTED;
    if (unit_f32act()) return launch_conv_split(a, opt_unit_dtype() == BMI_DTYPE_BF16X3, (hipStream_t)stream);     // (pair32 tensors, head / tail weight planes)
    const int rc = launch_conv3x3_s2(a, (hipStream_t)stream);      // the engine's order: conv3x3_s2 where it applies, else conv_igemm_wide
    return rc != BMI_ERR_UNSUPPORTED ? rc : launch_conv_igemm_wide(a, (hipStream_t)stream);
}

int bmi_conv3x3_shortcut_fwd(const void* in, const void* weight, const void* in2, const void* weight2, const float* bias,
                             void* out, int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t cin2,
                             int32_t relu, bmi_stream stream) {
    if (!in || !weight || !in2 || !weight2 || !out) return BMI_ERR_INVALID;
    ConvArgs a;
    std::memset(&a, 0, sizeof(a));
    a.bf16 = opt_unit_dtype() == BMI_DTYPE_BF16;
    a.in = (const _Float16*)in; a.wgt = (const _Float16*)weight; a.bias = bias; a.out = (_Float16*)out;
    a.N = n; a.in_mod = n; a.H = h; a.W = w; a.Cin = cin; a.Cout = cout; a.Ho = h; a.Wo = w;
    a.ksize = 3; a.stride = 1; a.pad = 1; a.relu = relu; a.M = n * h * w; a.B = n; a.out_mul = 1.f;
    a.in2 = (const _Float16*)in2; a.wgt2 = (const _Float16*)weight2; a.in2_mod = n; a.H2 = 2 * h; a.W2 = 2 * w;
    a.Cin2 = cin2; a.stride2 = 2;
    a.site = resolve_site(nullptr, 0, 0);
    if (opt_unit_dtype() == BMI_DTYPE_F32) return BMI_ERR_UNSUPPORTED;
    if (unit_f32act()) return launch_conv_split(a, opt_unit_dtype() == BMI_DTYPE_BF16X3, (hipStream_t)stream);     // (pair32 tensors, head / tail weight planes)
    return launch_conv(a, (hipStream_t)stream);     // conv3x3_pw where it applies, else conv3x3_patch
}

static int elt_args(EltArgs& a, const void* in, void* out, int n, int in_mod, int hw, int c, const bmi_site* site, int batch,
                    int t0, uint64_t seed, int cnt0) {
    if (!in || !out) return BMI_ERR_INVALID;
    if (site && !site_ok(*site)) return BMI_ERR_INVALID;
    std::memset(&a, 0, sizeof(a));
    a.bf16 = opt_unit_dtype() == BMI_DTYPE_BF16;
    a.in = (const _Float16*)in; a.out = out; a.N = n; a.in_mod = in_mod; a.HW = hw; a.C = c; a.B = batch; a.t0 = t0;
    a.site = resolve_site(site, seed, cnt0);
    return BMI_OK;
}

int bmi_mask_apply(const void* in, void* out, int32_t n, int32_t in_mod, int32_t hw, int32_t c, const bmi_site* site,
                   int32_t batch, int32_t t0, uint64_t seed, int32_t mask_cnt0, bmi_stream stream) {
    EltArgs a;
    const int rc = elt_args(a, in, out, n, in_mod, hw, c, site, batch, t0, seed, mask_cnt0);
    if (rc == BMI_OK && unit_f32act()) { a.pair = unit_pair(); return launch_mask_apply_f32(a, (hipStream_t)stream); }
    return rc != BMI_OK ? rc : launch_mask_apply(a, (hipStream_t)stream);
}

int bmi_maxpool2(const void* in, void* out, int32_t n, int32_t h, int32_t w, int32_t c, bmi_stream stream) {
    if (!in || !out) return BMI_ERR_INVALID;
    if (unit_f32act()) return launch_maxpool2_f32((const float*)in, (float*)out, n, h, w, c, (hipStream_t)stream, unit_pair());
    return launch_maxpool2((const _Float16*)in, (_Float16*)out, n, h, w, c, opt_unit_dtype() == BMI_DTYPE_BF16, (hipStream_t)stream);
}

int bmi_dense_f32(const void* in, int32_t in_is_f32, const float* weight, const float* bias, float* out, int32_t n,
                  int32_t in_mod, int32_t k, int32_t cout, int32_t relu, const bmi_site* site, int32_t batch, int32_t t0,
                  uint64_t seed, int32_t mask_cnt0, bmi_stream stream) {
    if (!in || !weight || !bias || !out) return BMI_ERR_INVALID;
    if (site && !site_ok(*site)) return BMI_ERR_INVALID;
    return launch_dense_f32(in, in_is_f32 ? 1 : (unit_pair() ? 2 + unit_pair() : (opt_unit_dtype() == BMI_DTYPE_BF16 ? 2 : 0)), weight, bias, out, n, in_mod, k, cout, relu, resolve_site(site, seed, mask_cnt0), batch,
                            t0, (hipStream_t)stream);
}

int bmi_head_fused(const void* in, int32_t in_is_f32, int32_t in_mod, int32_t hw, int32_t k, const float* weight_pad,
                   const float* bias, int32_t out_dim, const bmi_site* site, const bmi_site* site_logits, int32_t batch, int32_t t0,
                   int32_t tc, uint64_t seed, int32_t mask_cnt0, double* S1, double* S2, double* SL, bmi_stream stream) {
    if ((site && !site_ok(*site)) || (site_logits && !site_ok(*site_logits))) return BMI_ERR_INVALID;
    HeadArgs a;
    std::memset(&a, 0, sizeof(a));
    a.in = in;
    a.in_kind = in_is_f32 ? 1 : (unit_pair() ? 2 + unit_pair() : (opt_unit_dtype() == BMI_DTYPE_BF16 ? 2 : 0));
    a.in_mod = in_mod; a.HW = hw; a.K = k; a.B = batch; a.t0 = t0; a.tc = tc;
    a.w = weight_pad; a.bias = bias; a.C = out_dim;
    a.site = resolve_site(site, seed, mask_cnt0);
    a.site_logits = resolve_site(site_logits, seed, mask_cnt0);
    a.S1 = S1; a.S2 = S2; a.SL = SL;
    return launch_head_fused(a, (hipStream_t)stream);
}

// every field of HeadArgs from the caller's struct, as make_head_args fills it (b0 for the logits site, b0 * K as the feature site's offset)
int bmi_head_fused_ex(const bmi_head_ex* heads, int32_t n_heads, bmi_stream stream) {
    if (!heads || n_heads < 1 || n_heads > BMI_HEAD_PACK_MAX) return BMI_ERR_INVALID;
    HeadArgs list[BMI_HEAD_PACK_MAX];
    for (int i = 0; i < n_heads; ++i) {
        const bmi_head_ex& h = heads[i];
        if ((h.site && !site_ok(*h.site)) || (h.site_logits && !site_ok(*h.site_logits))) return BMI_ERR_INVALID;
        if (h.image_offset < 0 || h.k < 0 || (h.image_map && h.n_mapped <= 0)) return BMI_ERR_INVALID;
        if (h.logits && (h.batch <= 0 || h.out_dim <= 0 || h.logits_tstride < (size_t)h.batch * (size_t)h.out_dim)) return BMI_ERR_INVALID;   // rows would overlap
        const uint64_t soff = (uint64_t)h.image_offset * (uint64_t)h.k;
        if (h.site && (h.site->kind == BMI_SITE_ELEMENTWISE || h.site->kind == BMI_SITE_CHANNEL) && soff % 64 != 0) return BMI_ERR_UNSUPPORTED;
        HeadArgs& a = list[i];
        std::memset(&a, 0, sizeof(a));
        a.in = h.in;
        a.in_kind = h.in_is_f32 ? 1 : (unit_pair() ? 2 + unit_pair() : (opt_unit_dtype() == BMI_DTYPE_BF16 ? 2 : 0));
        a.in_mod = h.in_mod; a.HW = h.hw; a.K = h.k; a.B = h.batch; a.t0 = h.t0; a.tc = h.tc;
        a.w = h.weight_pad; a.bias = h.bias; a.C = h.out_dim;
        a.imap = h.image_map; a.Bc = h.image_map ? h.n_mapped : 0;
        a.site = resolve_site(h.site, h.seed, h.mask_cnt0, soff);
        a.site_logits = resolve_site(h.site_logits, h.seed, h.mask_cnt0);
        a.b0 = h.image_offset;
        a.S1 = h.S1; a.S2 = h.S2; a.SL = h.SL; a.SH = h.SH;
        a.logits = h.logits; a.logits_tstride = h.logits_tstride;
        a.part = h.scratch;
        a.inv_tau = h.inv_tau;
        a.vec_scale = h.vec_scale; a.vec_bias = h.vec_bias; a.mat = h.mat; a.mat_bias = h.mat_bias;
    }
    return n_heads == 1 ? launch_head_fused(list[0], (hipStream_t)stream) : launch_head_fused_multi(list, n_heads, (hipStream_t)stream);
}

}  // extern "C"
