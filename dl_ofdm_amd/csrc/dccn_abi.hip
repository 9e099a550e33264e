// libdccn.so -- C ABI over the gfx950 kernels (see include/dccn.h for the contract and the
// reference call site each entry point replaces).
#include "abi_impl.h"

namespace dccn {
thread_local int g_last_hip_error = 0;
thread_local ChainCtx tl_chain = {1, {{0, 0, 0, 0, 0, 0, 0, 0}}, {0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}};
StepTraceState g_step_trace;
thread_local unsigned long long* tl_stamp = nullptr;
thread_local bool tl_graph_capture = false;

thread_local int tl_whole_k = -1;
thread_local int tl_tune_depth = 0;
thread_local int tl_tune_vals[TUNE_COUNT];
TuneTable g_tune = {{{9}, {7}, {7}, {7}, {0}, {0}, {0}, {1}, {1}, {1}, {1}, {1}, {3}, {1}, {14}, {0}, {0}, {1}, {0}, {2}, {1}, {1}, {0}, {0}, {1}, {2}, {0}, {1}}};
std::atomic<int> g_whole_k_global{1};

// ---------------------------------------------------------------------------------------
// R0
// ---------------------------------------------------------------------------------------
static int norm_grid_x(int cols) { return ceil_div(ceil_div(cols, 4), 64); }
static int norm_grid_y(int batch) { return ceil_div(batch, kNormRowsPerBlock); }

int norm_fused_blocks(int cols) { return ceil_div(ceil_div(cols, 4 * kNormFusedCG), 8) * 8; }
// moments: per-chunk column sums of the two-pass form; power: R8 partial sums, two buffers (dccn_rx_buffers.norm_slot) of
// `slots` each, the larger of the two forms' block counts
struct NormWs {
    double *moments, *power;
    size_t slots;
    double* power_slot(int slot) const { return power + (slot ? slots : 0); }
};
static NormWs norm_carve(Carver& c, int batch, int cols) {
    const size_t a = (size_t)norm_grid_x(cols) * norm_grid_y(batch), b = (size_t)norm_fused_blocks(cols), slots = a > b ? a : b;
    double* moments = c.take<double>((size_t)kNormRowChunks * cols * 2);
    return NormWs{moments, c.take<double>(2 * slots), slots};
}
size_t norm_ws_bytes(int batch, int cols) { return carved_bytes([&](Carver& c) { norm_carve(c, batch, cols); }); }

bool norm_fused_ok(const float* x, const float* y, int batch, int cols) {
    return (cols % 4 == 0) && batch <= 128 * kNormFusedRPT && aligned16(x) && aligned16(y);
}

// want_power: also emit the per-block partial sums of the clipped power (R8); adam != nullptr: the
// optimizer bookkeeping of the fused training step rides on the first kernel
// where norm_impl leaves the R8 partial sums for a [batch, cols] input in workspace `ws` (no launch)
void norm_power_partials(int batch, int cols, void* ws, size_t ws_bytes, const float* x, const float* y,
                                PowerPartials* pp, int slot) {
    Carver c(ws, ws_bytes);
    pp->partial = norm_carve(c, batch, cols).power_slot(slot);
    pp->n = norm_fused_ok(x, y, batch, cols) ? norm_fused_blocks(cols) : norm_grid_x(cols) * norm_grid_y(batch);
    pp->denom = (double)batch * (double)(cols / 2);
}

int norm_impl(const float* x, float* y, float* mean, float* var, bool want_power, PowerPartials* pp, int batch,
                     int cols, float eps, float peak, dccn_adam_state* adam, dccn_adam_hparams hp, void* ws,
                     size_t ws_bytes, hipStream_t s, int slot) {
    if (!x || !y || batch <= 0 || cols <= 0 || (want_power && (cols & 1))) return DCCN_ERR_INVALID_ARG;
    if (ws_bytes < norm_ws_bytes(batch, cols) || !ws) return DCCN_ERR_WORKSPACE;
    Carver c(ws, ws_bytes);
    const NormWs w = norm_carve(c, batch, cols);
    double *partial = w.moments, *pw = w.power_slot(slot);
    const int gx = norm_grid_x(cols), gy = norm_grid_y(batch);
    if (norm_fused_ok(x, y, batch, cols)) {
        // the whole batch of a column strip fits in one block's registers: single pass, single launch
        const int blocks = norm_fused_blocks(cols);
        DCCN_LAUNCH_CHAINS_Z((norm_fused_kernel<kNormFusedCG, kNormFusedRPT>), dim3(blocks), dim3(128 * kNormFusedCG), 0, s,
                             x, y, batch, cols, eps, peak, want_power ? pw : nullptr, mean, var, adam, hp);
        DCCN_LAUNCH_CHECK();
        if (pp) {
            pp->partial = pw;
            pp->n = blocks;
            pp->denom = (double)batch * (double)(cols / 2);
        }
        return DCCN_OK;
    }
    DCCN_NO_CHAINS();
    hipLaunchKernelGGL(moments_kernel, dim3(gx, kNormRowChunks), dim3(64, 4), 0, s, x, batch, cols, partial, adam, hp);
    DCCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(normalise_kernel, dim3(gx, gy), dim3(64, 4), 0, s, x, y, partial, batch, cols, eps, peak,
                       want_power ? pw : nullptr, mean, var);
    DCCN_LAUNCH_CHECK();
    if (pp) {
        pp->partial = pw;
        pp->n = gx * gy;
        pp->denom = (double)batch * (double)(cols / 2);
    }
    return DCCN_OK;
}

// ---------------------------------------------------------------------------------------
// GEMM-shaped ops
// ---------------------------------------------------------------------------------------
GemmParams gp_zero() {
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.stamp = tl_stamp;         // non-null only while a StepTraceScope names the launch being built (common.h)
    return p;
}
int round_k(int K) { return ceil_div(K, 64) * 64; }
// the fast GEMM loaders use 32-bit byte offsets from a uniform base: operand must be < 2 GiB
static bool small_enough(long long rows, long long ld) { return rows * ld * 4 < (1LL << 31); }

// ---- one description per GEMM role: extents, leading dimensions, the whole-k klen, the slab distance of a weight gradient and
// the two vector-legality flags.  A site adds only what it alone knows: the output pointer or slab target, colsum, the klen
// of a split plan, nranges / koff, aux / out2 / out3, gC.
// may the fast loaders read the operand at p as vectors?  div: the divisibility its layout asks for
static bool vec_ok(const float* p, bool div, long long rows, long long ld) { return div && aligned16(p) && small_enough(rows, ld); }
// a site whose kernels have no scalar loaders refuses, before its first launch, operands that are not vector-legal
static bool vec_both(const GemmParams& p) { return p.vecA && p.vecB; }

// extents, leading dimensions and the whole-k klen of C[M,N] = A . B over a contraction of K
static GemmParams gemm_role(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc) {
    GemmParams p = gp_zero();
    p.A = A; p.B = B; p.C = C;
    p.M = M; p.N = N; p.K = K;
    p.lda = lda; p.ldb = ldb; p.ldc = ldc;
    p.klen = round_k(K);
    return p;
}
// y[M,N] = x[M,K] . w[K,N] + bias.  ldx > 0: x is a column window of a wider row-major matrix (row stride ldx)
static GemmParams dense_fwd_params(const float* x, const float* w, const float* bias, float* y, int M, int K, int N, int ldx = 0) {
    GemmParams p = gemm_role(x, w, y, M, N, K, ldx > 0 ? ldx : K, N, N);
    p.bias = bias;
    p.vecA = vec_ok(x, (K % 4 == 0) && (p.lda % 4 == 0), M, p.lda);      // KCONTIG: k extent K
    p.vecB = vec_ok(w, N % 4 == 0, K, N);                                 // ICONTIG: ld = N, i extent N
    return p;
}
// dx[M,K] = dy[M,N] . w[K,N]^T
static GemmParams dense_bwd_x_params(const float* dy, const float* w, float* dx, int M, int K, int N) {
    GemmParams p = gemm_role(dy, w, dx, M, K, N, N, N, K);
    p.vecA = vec_ok(dy, N % 4 == 0, M, N);
    p.vecB = vec_ok(w, N % 4 == 0, K, N);
    return p;
}
// dw[K,N] = x[M,K]^T . dy[M,N].  ldx as dense_fwd_params
static GemmParams dense_bwd_w_params(const float* x, const float* dy, int M, int K, int N, int ldx = 0) {
    GemmParams p = gemm_role(x, dy, nullptr, K, N, M, ldx > 0 ? ldx : K, N, N);
    p.slab = (long long)K * N;
    p.vecA = vec_ok(x, (K % 4 == 0) && (p.lda % 4 == 0), M, p.lda);
    p.vecB = vec_ok(dy, N % 4 == 0, M, N);
    return p;
}
// out[rows,2F] = x[rows,2kin] . Weff[2kin,2F] + bias.  ldx: row stride of x; ldc: row stride of out (the joined pairs)
static GemmParams cconv_fwd_params(const float* x, const float* w, const float* bias, float* out, int rows, int kin, int F,
                                   int ldx = 0, int ldc = 0) {
    GemmParams p = gemm_role(x, w, out, rows, 2 * F, 2 * kin, ldx > 0 ? ldx : 2 * kin, 2 * F, ldc > 0 ? ldc : 2 * F);
    p.bias = bias; p.cbias = 1; p.cF = F;
    p.vecA = vec_ok(x, (kin % 2 == 0) && (p.lda % 4 == 0), rows, p.lda);
    p.vecB = vec_ok(w, F % 2 == 0, kin, 2LL * F);                         // float2 loads of [Wa|Wb] rows
    return p;
}
// dx[rows,2kin] = dout[rows,2F] . Weff^T.  ldc: row stride of dx
static GemmParams cconv_bwd_x_params(const float* dout, const float* w, float* dx, int rows, int kin, int F, int ldc = 0) {
    GemmParams p = gemm_role(dout, w, dx, rows, 2 * kin, 2 * F, 2 * F, 2 * F, ldc > 0 ? ldc : 2 * kin);
    p.cF = F;
    p.vecA = vec_ok(dout, F % 2 == 0, rows, 2LL * F);
    p.vecB = vec_ok(w, F % 2 == 0, kin, 2LL * F);
    return p;
}
// dWeff[2kin,2F] = x[rows,2kin]^T . dout[rows,2F]
static GemmParams cconv_bwd_w_params(const float* x, const float* dout, int rows, int kin, int F) {
    GemmParams p = gemm_role(x, dout, nullptr, 2 * kin, 2 * F, rows, 2 * kin, 2 * F, 2 * F);
    p.slab = 4LL * kin * F;
    p.vecA = vec_ok(x, kin % 2 == 0, rows, 2LL * kin);
    p.vecB = vec_ok(dout, F % 2 == 0, rows, 2LL * F);
    return p;
}

// ---- one table per variant family (Tile16Cfg, abi_impl.h): a family's launcher is a template over the variant number that
// reads its row; a table of its instantiations, indexed by the variant, sits next to the rows

// ---- the launch an operator issues, decided ONCE per operator by its *_route function: the *_impl function issues what the
// route names, dccn_gemm_route_query reports it (include/dccn.h: dccn_gemm_route, the DCCN_FAMILY_* ids).  A route function
// returns DCCN_ERR_INVALID_ARG where the operator refuses -- before any launch.
using Route = dccn_gemm_route;
enum RouteStage : int { STAGE_SPLIT_PAIRS = 6 };      // (after the StoreStage values: the dX stores of a concat's gradient)
static Route route_of(int family, int variant, int rows, int cols, int bk) {
    Route r;
    memset(&r, 0, sizeof(r));
    r.family = family; r.variant = variant;
    r.tile_rows = rows; r.tile_cols = cols; r.tile_k = bk;
    r.splits = 1; r.stage = STORE_PLAIN;
    return r;
}
static Route route16(int family, int variant, const Tile16Cfg& c) { return route_of(family, variant, c.rows(), c.cols(), c.bk); }
static Route with_split(Route r, const SplitPlan& sp) {
    r.splits = sp.splits; r.klen = sp.klen;
    return r;
}
// the tile launch_gemm picks (gemm_f32_mfma.h)
template <int KA, int KB>
static Route route_generic(const GemmParams& p, int splits = 1) {
    const GemmTile t = gemm_tile<KA, KB>(p, splits);
    Route r = route_of(DCCN_FAMILY_GENERIC, 0, t.bm, t.bn, t.bk);
    r.splits = splits; r.klen = p.klen;
    return r;
}
// the one-latency 16x16 tiles of fewrow.h: ng slots of 64 k each
static Route route_fewrow(int ng) { return route_of(DCCN_FAMILY_FEWROW, 0, 16, 16, 64 * ng); }

// the tiles the plain and the fused (tail / decision) dense forward run on: 48x64 with loads two k-tiles ahead (small layers),
// 80x64 (large layers), 32x64 for a short last tile row next to the 80x64 tiles
constexpr Tile16Cfg kDense48 = {1, 4, 3, 1, 64, 1}, kDense80 = {1, 4, 5, 1, 64, 1}, kDense32 = {1, 4, 2, 1, 64, 1};
static_assert(kDense48.cols() == 64 && kDense80.cols() == 64 && kDense32.cols() == 64 && kDense48.bk == kDense80.bk &&
              kDense32.bk == kDense80.bk, "the fused dense forward kernels are written for 1 x 4 waves of TM x 1 tiles");
// ACT: element-wise stage in the store (2 = tanh, 5 = the equaliser stage)
template <int ACT = 1>
static int dense48_launch(const GemmParams& p, hipStream_t s, size_t smem_min = 0) {
    constexpr Tile16Cfg c = kDense48;
    return launch_gemm16<OP_KCONTIG, OP_ICONTIG, c.wgm, c.wgn, c.tm, c.tn, c.bk, c.ks, 0, TAG_DENSE_FWD, 2, ACT>(p, 1, s, smem_min);
}

// asked: the element-wise stage the caller asks for; route.stage: the one the launch carries -- a tile family carries stages
// from a level of knob 19 on: the few-row and skinny tiles from level 1, the 48x64 tiles from level 2
static int dense_fwd_route(const GemmParams& p, int asked, Route* out) {
    const auto stage_from = [&](int level) { return g_tune[TUNE_EQ_EPILOGUES] >= level ? asked : (int)STORE_PLAIN; };
    // few rows, K = 640 / 896: every operand of a 16x16 tile requested at once, no LDS staging (fewrow.h)
    if (g_tune[TUNE_FEWROW] && g_tune[TUNE_SKINNY] > 0 && fewrow_ng(p) && aligned16(p.C)) {
        *out = route_fewrow(fewrow_ng(p));
        out->stage = stage_from(1);
    } else if (skinny_ok(p)) {
        // (a stage runs on variant 1 whatever the knob says)
        const int st = stage_from(1), v = st != STORE_PLAIN ? 1 : g_tune[TUNE_SKINNY];
        if (v > kSkinnyVariants) return DCCN_ERR_INVALID_ARG;
        *out = route16(DCCN_FAMILY_SKINNY, v, kSkinny16[v]);
        out->stage = st;
    } else if (g_tune[TUNE_DENSE_FWD_PLAIN] && vec_both(p) && (p.K % 4 == 0) && (p.N % 4 == 0) && p.K >= 128 &&
               (long long)ceil_div(p.M, 128) * ceil_div(p.N, 128) < 2 * kCUs) {
        // small layers (64x64 tiles would leave CUs without a block: 1170x640 = 190 tiles): the 48x64 tiles of the fused
        // kernel, loads two k-tiles ahead
        *out = route16(DCCN_FAMILY_GEMM16, 0, kDense48);
        out->stage = stage_from(2);
    } else {
        *out = route_generic<OP_KCONTIG, OP_ICONTIG>(p);
    }
    return DCCN_OK;
}

// ldx: as dense_fwd_params
// act = 2: y = tanh(x.w + bias) when the launch plan has the stage (few-row 16x64 tiles); *act_done tells
// act = 5 (+ aux = the received cells, out2 / out3): the output is a channel estimate; eq and corr of model.py:431-438
// leave the same launch
int dense_fwd_impl(const float* x, const float* w, const float* bias, float* y, int M, int K, int N,
                          hipStream_t s, int ldx, int act, bool* act_done, const float* aux,
                          float* out2, float* out3) {
    if (act_done) *act_done = false;
    if (!x || !w || !y || M <= 0 || K <= 0 || N <= 0) return DCCN_ERR_INVALID_ARG;
    GemmParams p = dense_fwd_params(x, w, bias, y, M, K, N, ldx);
    const bool eq_stage = act == 5 && act_done && aux && out2 && out3 && g_tune[TUNE_EQ_EPILOGUES] && (N % 2 == 0) &&
                          aligned16(aux) && aligned16(out2) && aligned16(out3);
    if (eq_stage) { p.aux = aux; p.out2 = out2; p.out3 = out3; }
    // the element-wise stage the caller asks for (dense_fwd_route: which one the launch carries)
    const int asked = eq_stage ? 5 : (act == 2 && act_done) ? 2 : 1;
    Route r;
    DCCN_TRY(dense_fwd_route(p, asked, &r));
    if (r.stage != STORE_PLAIN) *act_done = true;       // set exactly when the launch carries a stage
    switch (r.family) {
        case DCCN_FAMILY_FEWROW: switch (r.stage) {
            case 5: return launch_fewrow<OP_ICONTIG, 5, TAG_DENSE_FWD>(p, s);
            case 2: return launch_fewrow<OP_ICONTIG, 2, TAG_DENSE_FWD>(p, s);
            default: return launch_fewrow<OP_ICONTIG, 1, TAG_DENSE_FWD>(p, s);
        }
        case DCCN_FAMILY_SKINNY: switch (r.stage) {
            case 5: return skinny_launch<OP_KCONTIG, OP_ICONTIG, TAG_DENSE_FWD, 5>(r.variant, p, s);
            case 2: return skinny_launch<OP_KCONTIG, OP_ICONTIG, TAG_DENSE_FWD, 2>(r.variant, p, s);
            default: return skinny_launch<OP_KCONTIG, OP_ICONTIG, TAG_DENSE_FWD>(r.variant, p, s);
        }
        case DCCN_FAMILY_GEMM16: switch (r.stage) {
            case 5: return dense48_launch<5>(p, s);
            case 2: return dense48_launch<2>(p, s);
            default: return dense48_launch<1>(p, s);
        }
        default: return launch_gemm<OP_KCONTIG, OP_ICONTIG, 0, TAG_DENSE_FWD>(p, 1, s);
    }
}

// (p.C = dx: the few-row tiles ask for an output)
static int dense_bwd_x_route(const GemmParams& p, Route* out) {
    if (g_tune[TUNE_FEWROW] && g_tune[TUNE_SKINNY] > 0 && fewrow_ng(p)) {
        *out = route_fewrow(fewrow_ng(p));
    } else if (skinny_ok(p)) {
        const int v = g_tune[TUNE_SKINNY];
        if (v > kSkinnyVariants) return DCCN_ERR_INVALID_ARG;
        *out = route16(DCCN_FAMILY_SKINNY, v, kSkinny16[v]);
    } else {
        *out = route_generic<OP_KCONTIG, OP_KCONTIG>(p);
    }
    return DCCN_OK;
}
int dense_bwd_x_impl(const float* dy, const float* w, float* dx, int M, int K, int N, hipStream_t s) {
    if (!dy || !w || !dx || M <= 0 || K <= 0 || N <= 0) return DCCN_ERR_INVALID_ARG;
    const GemmParams p = dense_bwd_x_params(dy, w, dx, M, K, N);
    Route r;
    DCCN_TRY(dense_bwd_x_route(p, &r));
    switch (r.family) {
        case DCCN_FAMILY_FEWROW: return launch_fewrow<OP_KCONTIG, 1, TAG_DENSE_BWD_X>(p, s);
        case DCCN_FAMILY_SKINNY: return skinny_launch<OP_KCONTIG, OP_KCONTIG, TAG_DENSE_BWD_X>(r.variant, p, s);
        default: return launch_gemm<OP_KCONTIG, OP_KCONTIG, 0, TAG_DENSE_BWD_X>(p, 1, s);
    }
}

// slab capacity for the weight-gradient split-K plans: small outputs may be cut into up to 8 k ranges (gemm16 paths)
static int max_splits16(int Mo, int No) {
    const long long tiles = (long long)ceil_div(Mo, 64) * ceil_div(No, 64);
    long long m = (1024 + tiles - 1) / tiles;
    return (int)(m < 1 ? 1 : (m > 8 ? 8 : m));
}
// The slab workspaces are sized for a capacity and carved for the count a launch planned: false when that count does not fit
// the caller's bytes (every site returns DCCN_ERR_WORKSPACE then, before its first launch)
bool slab_carve(Carver& c, int splits, int Mo, int No, SlabWs* w) {
    w->splits = splits;
    w->slab = (long long)Mo * No;
    w->slabs = c.take<float>((size_t)splits * Mo * No);
    w->colsum = c.take<float>((size_t)splits * No);
    return c.ok();
}
static int splitk_capacity(int Mo, int No, int Kr) {
    const int planned = plan_splitk(Mo, No, Kr).splits, ms = max_splits16(Mo, No);
    return planned > ms ? planned : ms;
}
size_t splitk_ws_bytes(int Mo, int No, int Kr) {
    SlabWs w;
    return carved_bytes([&](Carver& c) { slab_carve(c, splitk_capacity(Mo, No, Kr), Mo, No, &w); });
}
// what a weight-gradient launch leaves for the launch that sums its slabs.  live = false: it wrote the gradient itself (a single
// k range outside the fused backward launch, whose dW items always write slabs)
static DeferredSlabs deferred_slabs(const SlabWs& w, bool bias, bool live) {
    return live ? DeferredSlabs{w.slabs, bias ? w.colsum : nullptr, w.splits} : DeferredSlabs{nullptr, nullptr, 1};
}
static FoldDefer fold_defer(const SlabWs& w) { return FoldDefer{w.slabs, w.colsum, w.splits, w.slab}; }

// split plan of the dense weight gradient dw[K,N] = x[M,K]^T . dy[M,N] (one rule for the stand-alone operator and the
// grouped launch: the composed and the fused step must sum in the same order)
// range_rows: preferred k-range length of the k-major form.  256 (4 k-tiles) next to plain dX tiles: the blocks are cheap
// to start and pack the grid's tail better than the 320-row ranges of the generic plan (C2: 5 ranges instead of 4, -1 us
// per step even with one more slab to sum).  448 (7 k-tiles) in the fused backward launch of rx_bwd.h, whose dX tiles carry
// the C-Conv contraction and run 26 us: fewer, longer dW items amortise their load/store phases and leave two slabs less
// for the optimizer launch (C2: 3 ranges, -2.0 us per step; 2, 4 and 6 ranges measured +1.2 ... +1.5 us over 3).
static SplitPlan dense_dw_plan(int M, int K, int N, int range_rows = 256) {
    SplitPlan sp = plan_splitk(K, N, M);
    const int cap = max_splits16(K, N);
    if (g_tune[TUNE_DENSE_BWD_SPLITS] > 0 && sp.splits > 1) {
        sp = plan_splitk_n(M, g_tune[TUNE_DENSE_BWD_SPLITS] < cap ? g_tune[TUNE_DENSE_BWD_SPLITS] : cap, 64);
    } else if (g_tune[TUNE_DENSE_BWD] == kVariantKmajor && sp.splits > 1 && (range_rows > 256 || sp.klen > range_rows)) {
        const int want = ceil_div(M, range_rows);
        const SplitPlan alt = plan_splitk_n(M, want < cap ? want : cap, 64);
        if (range_rows > 256 || alt.splits > sp.splits) sp = alt;
    }
    return sp;
}
constexpr int kFusedBwdRangeRows = 448;
// graded k ranges (in 64-row k-tiles, as shares of the total): the items are dispatched range by range, so the last ones
// handed out are the short ones
static int graded_ranges(int preset, int M, int off[9]) {
    static const int shares[][8] = {{0}, {8, 6, 3, 2, 0}, {9, 6, 4, 0}, {7, 5, 4, 3, 0}, {10, 9, 0}, {8, 7, 4, 0}, {6, 5, 4, 3, 1, 0},
                                    {9, 7, 3, 0}, {9, 6, 3, 1, 0}, {8, 5, 3, 2, 1, 0}, {10, 5, 3, 1, 0}, {7, 6, 4, 2, 0},
                                    {8, 6, 4, 1, 0}, {9, 5, 3, 2, 0}, {9, 5, 2, 2, 1, 0}, {8, 4, 3, 2, 2, 0}, {10, 4, 2, 2, 1, 0},
                                    {7, 5, 3, 2, 2, 0}, {9, 4, 3, 2, 1, 0}, {8, 5, 3, 1, 2, 0}, {7, 5, 4, 2, 1, 0},
                                    {8, 4, 3, 2, 1, 1, 0}, {9, 4, 2, 2, 1, 1, 0}, {9, 5, 2, 1, 1, 1, 0}, {10, 4, 2, 1, 1, 1, 0}};
    if (preset < 1 || preset > 24) return 0;
    const int nt = ceil_div(M, 64);
    int tot = 0, n = 0;
    while (shares[preset][n]) tot += shares[preset][n++];
    int used = 0, acc = 0, cnt = 0;
    off[0] = 0;
    for (int i = 0; i < n; ++i) {
        acc += shares[preset][i];
        int upto = (int)((long long)acc * nt / tot);
        if (i == n - 1) upto = nt;
        if (upto <= used) continue;
        used = upto;
        off[++cnt] = upto * 64 < M ? upto * 64 : M;
    }
    return cnt;
}

// the stand-alone dense weight gradient under split plan sp.  p.C = the slabs, p.klen = sp.klen
static Route dense_bwd_w_route(const GemmParams& p, const SplitPlan& sp) {
    const long long big = (long long)ceil_div(p.M, 128) * ceil_div(p.N, 128) * sp.splits;
    if (sp.splits > 1 && g_tune[TUNE_DENSE_BWD] == kVariantKmajor && kmajor_ok(p) && big < 2 * kCUs)
        return with_split(route_of(DCCN_FAMILY_KMAJOR, 0, 64, 64, 64), sp);
    return route_generic<OP_ICONTIG, OP_ICONTIG>(p, sp.splits);
}
// defer != nullptr: leave the split-K slabs un-reduced (the fused Adam kernel sums them) and report them
int dense_bwd_w_impl(const float* x, const float* dy, float* dw, float* dbias, int M, int K, int N, void* ws,
                            size_t ws_bytes, hipStream_t s, DeferredSlabs* defer, int ldx) {
    if (!x || !dy || !dw || M <= 0 || K <= 0 || N <= 0) return DCCN_ERR_INVALID_ARG;
    if (!ws || ws_bytes < splitk_ws_bytes(K, N, M)) return DCCN_ERR_WORKSPACE;
    const SplitPlan sp = dense_dw_plan(M, K, N);
    Carver c(ws, ws_bytes);
    SlabWs sw;
    if (!slab_carve(c, sp.splits, K, N, &sw)) return DCCN_ERR_WORKSPACE;
    GemmParams p = dense_bwd_w_params(x, dy, M, K, N, ldx);
    p.klen = sp.klen;
    p.C = sw.slabs;
    const Route r = dense_bwd_w_route(p, sp);
    if (defer) *defer = deferred_slabs(sw, false, false);
    if (sp.splits == 1) {
        p.C = dw;
        p.colsum = dbias;
        return launch_gemm<OP_ICONTIG, OP_ICONTIG, 1, TAG_DENSE_BWD_W>(p, 1, s);
    }
    p.colsum = dbias ? sw.colsum : nullptr;
    if (r.family == DCCN_FAMILY_KMAJOR)
        DCCN_TRY((launch_kmajor<1, TAG_DENSE_BWD_W>(p, sp.splits, s)));
    else
        DCCN_TRY((launch_gemm<OP_ICONTIG, OP_ICONTIG, 1, TAG_DENSE_BWD_W>(p, sp.splits, s)));
    if (defer) {
        *defer = deferred_slabs(sw, dbias != nullptr, true);
        return DCCN_OK;
    }
    const long long n = (long long)K * N;
    if (dbias) DCCN_TRY(launch_splitk_reduce2(sw.slabs, sp.splits, n, dw, n, sw.colsum, (long long)N, dbias, (long long)N, s));
    else DCCN_TRY(launch_splitk_reduce(sw.slabs, sp.splits, n, dw, n, s));
    return DCCN_OK;
}

// TUNE_DENSE_BWD 1-6: the dX and the dW tiles of the grouped gemm16 launch (one k-tile depth for both: x.bk)
struct DenseBwd16Cfg { Tile16Cfg x, w; };
constexpr int kDenseBwd16Rows = 6;
constexpr DenseBwd16Cfg kDenseBwd16[kDenseBwd16Rows + 1] = {{},
    {{2, 2, 2, 2, 32, 1}, {2, 2, 2, 2, 32, 1}},     // dX 64x64, dW 64x64
    {{1, 4, 3, 1, 32, 1}, {2, 2, 2, 2, 32, 1}},     // dX 48x64
    {{2, 2, 2, 2, 64, 1}, {2, 2, 2, 2, 64, 1}},     // 64-deep k-tiles
    {{2, 2, 3, 2, 32, 1}, {2, 2, 2, 2, 32, 1}},     // dX 96x64
    {{2, 2, 2, 4, 32, 1}, {2, 2, 2, 4, 32, 1}},     // 64x128 both
    {{2, 2, 2, 2, 32, 1}, {2, 2, 2, 4, 32, 1}}};    // dX 64x64, dW 64x128
template <int V>
static int dense_bwd16_launch(const GemmParams& px, const GemmParams& pw, int splits, hipStream_t s) {
    constexpr Tile16Cfg x = kDenseBwd16[V].x, w = kDenseBwd16[V].w;
    static_assert(x.bk == w.bk, "one k-tile depth for the dX and the dW tiles");
    return launch_dense_bwd16<x.wgm, x.wgn, x.tm, x.tn, x.bk, w.wgm, w.wgn, w.tm, w.tn>(px, pw, splits, s, tune_smem_min());
}
constexpr int (*kDenseBwd16Launch[7])(const GemmParams&, const GemmParams&, int, hipStream_t) = {nullptr,
    dense_bwd16_launch<1>, dense_bwd16_launch<2>, dense_bwd16_launch<3>, dense_bwd16_launch<4>, dense_bwd16_launch<5>, dense_bwd16_launch<6>};
// few rows: dX on the 16x64 skinny tiles, the unsplit dW on 64x64 tiles.  STAGE: element-wise stage of the dX stores
constexpr DenseBwd16Cfg kDenseBwdSkinny = {kSkinny16[1], {2, 2, 2, 2, 64, 1}};
template <int STAGE>
static int dense_bwd_skinny_launch(const GemmParams& px, const GemmParams& pw, hipStream_t s) {
    constexpr Tile16Cfg x = kDenseBwdSkinny.x, w = kDenseBwdSkinny.w;
    return launch_dense_bwd16<x.wgm, x.wgn, x.tm, x.tn, x.bk, w.wgm, w.wgn, w.tm, w.tn, STAGE>(px, pw, 1, s, tune_smem_min());
}

// px, pw as dense_bwd_x_params / dense_bwd_w_params build them, pw.C = where the slabs will lie (the head of the workspace).
// actx: the element-wise stage the caller asks of the dX stores (1 = none, 3 = times (1 - aux^2), 4 = plus aux); split_pairs:
// dx is the gradient of a concat of two IQ-pair streams and the caller asks the stores to write the streams' own buffers.
// route.splits / klen: the split plan of dW; route.stage: what the dX stores carry.
static int dense_bwd_route(const GemmParams& px, GemmParams pw, int M, int K, int N, int actx, bool split_pairs, Route* out) {
    const bool vec = vec_both(px) && vec_both(pw);
    // few rows (the equaliser's 73-frame batch): dX on 16x64 tiles and the unsplit dW (k = the few rows: one or two
    // k-tiles) in ONE grid -- round 2 ran them as two launches of 6-10 us each, almost all of it launch ramp and drain
    if (g_tune[TUNE_SKINNY] > 0 && g_tune[TUNE_SKINNY_GROUPED] && vec && M <= 96 && (K % 4 == 0) && (N % 4 == 0)) {
        const int ng = g_tune[TUNE_FEWROW] ? fewrow_ng(px) : 0;       // dX on the one-latency 16x16 tiles of fewrow.h
        Route r = ng ? route_fewrow(ng) : route16(DCCN_FAMILY_SKINNY, 1, kDenseBwdSkinny.x);
        r.w_tile_rows = kDenseBwdSkinny.w.rows(); r.w_tile_cols = kDenseBwdSkinny.w.cols();
        r.klen = pw.klen;                                             // (the few rows, as built)
        if (actx != 1 && g_tune[TUNE_EQ_EPILOGUES]) {
            if (actx != 3 && actx != 4) return DCCN_ERR_INVALID_ARG;
            r.stage = actx;
        }
        *out = r;
        return DCCN_OK;
    }
    const int variant = g_tune[TUNE_DENSE_BWD] == kVariantKmajor ? 0 : g_tune[TUNE_DENSE_BWD];
    const long long big = (long long)ceil_div(M, 128) * ceil_div(K, 128);
    if (variant > 0 && vec && big < 2 * kCUs) {
        if (variant > kDenseBwd16Rows) return DCCN_ERR_INVALID_ARG;       // (no such row)
        const Tile16Cfg cx = kDenseBwd16[variant].x, cw = kDenseBwd16[variant].w;
        const int nx = ceil_div(px.M, cx.rows()) * ceil_div(px.N, cx.cols()), tw = ceil_div(pw.M, cw.rows()) * ceil_div(pw.N, cw.cols());
        int want = g_tune[TUNE_DENSE_BWD_SPLITS];
        if (want <= 0) want = (3 * kCUs - nx + tw / 2) / tw;            // about three resident blocks per CU in all
        const int cap = max_splits16(K, N);
        if (want > cap) want = cap;
        Route r = with_split(route16(DCCN_FAMILY_GEMM16, variant, cx), plan_splitk_n(M, want, cx.bk));
        r.w_tile_rows = cw.rows(); r.w_tile_cols = cw.cols();
        *out = r;
        return DCCN_OK;
    }
    const SplitPlan sp = dense_dw_plan(M, K, N);
    pw.klen = sp.klen;
    Route r;
    if (vec && g_tune[TUNE_DENSE_BWD_BIG] && grouped_big_ok(px, pw, sp.splits)) {
        r = route_of(DCCN_FAMILY_GROUPED_BIG, 0, 128, 128, 32);
        r.w_tile_rows = r.w_tile_cols = 128;
    } else if (sp.splits < 2 || !vec || !grouped_ok(px, pw, sp.splits)) {
        r = route_of(DCCN_FAMILY_TWO_LAUNCH, 0, 0, 0, 0);
    } else {
        pw.ldc = N;
        const bool km = g_tune[TUNE_DENSE_BWD] == kVariantKmajor && kmajor_ok(pw);
        r = route_of(km ? DCCN_FAMILY_GROUPED_KMAJOR : DCCN_FAMILY_GROUPED, 0, 64, 64, 64);
        r.w_tile_rows = r.w_tile_cols = 64;
        if (km && split_pairs && (K % 4 == 0)) {
            r.stage = STAGE_SPLIT_PAIRS;
        } else if (km && actx != 1 && g_tune[TUNE_EQ_EPILOGUES] >= 2) {
            if (actx != 3 && actx != 4) return DCCN_ERR_INVALID_ARG;
            r.stage = actx;
        }
    }
    *out = with_split(r, sp);
    return DCCN_OK;
}

// dense backward as ONE grouped launch: dx = dy.w^T together with the split-K slabs of dw = x^T.dy
// (left un-reduced for the fused Adam kernel).  Falls back to two launches when the grouped
// configuration does not apply (128x128 tiles, unaligned operands, single split).
int dense_bwd_grouped_impl(const float* x, const float* dy, const float* w, float* dx, float* dw, float* dbias,
                                  int M, int K, int N, void* ws, size_t ws_bytes, hipStream_t s, DeferredSlabs* defer,
                                  int actx, const float* aux, bool* act_done,
                                  float* split_dst, long long split_pairs_gc, bool* split_done) {
    if (act_done) *act_done = false;
    if (split_done) *split_done = false;
    if (!x || !dy || !w || !dx || !dw || !defer || M <= 0 || K <= 0 || N <= 0) return DCCN_ERR_INVALID_ARG;
    if (!ws || ws_bytes < splitk_ws_bytes(K, N, M)) return DCCN_ERR_WORKSPACE;
    GemmParams px = dense_bwd_x_params(dy, w, dx, M, K, N);
    GemmParams pw = dense_bwd_w_params(x, dy, M, K, N);       // (klen: the whole k range until a branch plans its split)
    Route r;
    {
        GemmParams pq = pw;
        pq.C = static_cast<float*>(ws);             // (slab_carve's first piece lies at the head of the workspace)
        DCCN_TRY(dense_bwd_route(px, pq, M, K, N, (act_done && aux) ? actx : 1, split_done && split_dst && split_pairs_gc != 0, &r));
    }
    // the dX tiles may carry an element-wise stage of the caller's graph: 3 = times (1 - aux^2) (tanh gradient),
    // 4 = plus aux (gradient accumulation): two 5 us launches of the equaliser step less
    if (r.stage == STORE_TANHGRAD || r.stage == STORE_ADD) {
        px.aux = aux;
        *act_done = true;
    }
    if (r.family == DCCN_FAMILY_FEWROW || r.family == DCCN_FAMILY_SKINNY) {
        pw.C = dw; pw.colsum = dbias; pw.slab = 0;       // (klen = the few rows, as built)
        const bool few = r.family == DCCN_FAMILY_FEWROW;
        if (r.stage == STORE_TANHGRAD) DCCN_TRY(few ? launch_dense_bwd_fewrow<3>(px, pw, s) : dense_bwd_skinny_launch<3>(px, pw, s));
        else if (r.stage == STORE_ADD) DCCN_TRY(few ? launch_dense_bwd_fewrow<4>(px, pw, s) : dense_bwd_skinny_launch<4>(px, pw, s));
        else DCCN_TRY(few ? launch_dense_bwd_fewrow<1>(px, pw, s) : dense_bwd_skinny_launch<1>(px, pw, s));
        *defer = deferred_slabs(SlabWs{}, false, false);
        return DCCN_OK;
    }
    if (r.family == DCCN_FAMILY_TWO_LAUNCH) {
        DCCN_TRY(dense_bwd_w_impl(x, dy, dw, dbias, M, K, N, ws, ws_bytes, s, defer));
        return dense_bwd_x_impl(dy, w, dx, M, K, N, s);
    }
    Carver c(ws, ws_bytes);
    SlabWs sw;
    if (!slab_carve(c, r.splits, K, N, &sw)) return DCCN_ERR_WORKSPACE;
    pw.C = sw.slabs; pw.colsum = dbias ? sw.colsum : nullptr;
    pw.klen = r.klen;
    if (r.family == DCCN_FAMILY_GEMM16) {
        if (r.splits == 1) { pw.C = dw; pw.colsum = dbias; }
        DCCN_TRY(kDenseBwd16Launch[r.variant](px, pw, r.splits, s));
        *defer = deferred_slabs(sw, dbias != nullptr, r.splits > 1);
        return DCCN_OK;
    }
    pw.ldc = N;
    if (r.family == DCCN_FAMILY_GROUPED_BIG) {
        if (r.splits == 1) { pw.C = dw; pw.colsum = dbias; pw.slab = 0; }
        DCCN_TRY((launch_dense_bwd_grouped<true, 128, 128, 32>(px, pw, r.splits, s)));
        *defer = deferred_slabs(sw, dbias != nullptr, r.splits > 1);
        return DCCN_OK;
    }
    if (r.family == DCCN_FAMILY_GROUPED_KMAJOR) {
        if (r.stage == STAGE_SPLIT_PAIRS) {
            // dx is the gradient of a concat of two IQ-pair streams: the stores write the two streams' own buffers
            // instead of dx (split_dst = stream 0, [M, K/2]; stream 1 split_pairs_gc elements further)
            px.C = split_dst; px.ldc = K / 2; px.gC = split_pairs_gc;
            *split_done = true;
            DCCN_TRY((launch_dense_bwd_grouped_km<64, CMAP_SPLIT_PAIRS>(px, pw, r.splits, s)));
        }
        else if (r.stage == STORE_TANHGRAD) DCCN_TRY((launch_dense_bwd_grouped_km<64, CMAP_TANHGRAD>(px, pw, r.splits, s)));
        else if (r.stage == STORE_ADD) DCCN_TRY((launch_dense_bwd_grouped_km<64, CMAP_ADD>(px, pw, r.splits, s)));
        else DCCN_TRY(launch_dense_bwd_grouped_km<64>(px, pw, r.splits, s));
    } else DCCN_TRY(launch_dense_bwd_grouped<true>(px, pw, r.splits, s));
    *defer = deferred_slabs(sw, dbias != nullptr, true);
    return DCCN_OK;
}

// TUNE_CCONV_FWD 1-6: gemm16 tiles of the C-Conv forward
constexpr int kCconvFwd16Rows = 6;
constexpr Tile16Cfg kCconvFwd16[kCconvFwd16Rows + 1] = {{},
    {2, 2, 1, 4, 32, 1},      // 32x128
    {1, 4, 2, 2, 32, 1},      // 32x128, wave 32x32
    {1, 4, 1, 2, 32, 1},      // 16x128
    {2, 2, 2, 2, 32, 1},      // 64x64
    {1, 4, 1, 2, 32, 2},      // 16x128, 8 waves
    {2, 2, 1, 2, 32, 1}};     // 32x64
template <int V>
static int cconv_fwd16_launch(const GemmParams& p, hipStream_t s) {
    constexpr Tile16Cfg c = kCconvFwd16[V];
    return launch_gemm16<OP_KCONTIG, OP_CCONV_W, c.wgm, c.wgn, c.tm, c.tn, c.bk, c.ks, 0, TAG_CCONV_FWD>(p, 1, s, tune_smem_min());
}
constexpr int (*kCconvFwd16Launch[7])(const GemmParams&, hipStream_t) = {nullptr,
    cconv_fwd16_launch<1>, cconv_fwd16_launch<2>, cconv_fwd16_launch<3>, cconv_fwd16_launch<4>, cconv_fwd16_launch<5>, cconv_fwd16_launch<6>};
// (a value past 11 runs the 32x32x2 family, as 0 does: no table is indexed with it)
static Route cconv_fwd_route(const GemmParams& p, int kin) {
    const int variant = g_tune[TUNE_CCONV_FWD];
    const long long big = (long long)ceil_div(p.M, 128) * ceil_div(p.N, 128);
    // 7-11 (default 7): the staged whole-k tile of cconv_fwd.h (K = 160 / 128, i.e. N = 64 with / without the cyclic
    // prefix): bit-identical to the whole-k tile of gemm_f32_mfma.h it replaces; 8 / 9 = other LDS-store slots
    // 10 / 11: 32 x 128 tiles (every x row read by one block)
    if (variant >= 7 && variant <= 11 && big < 2 * kCUs && cconv_fwd_staged_ok(p))
        return variant >= 10 ? route_of(DCCN_FAMILY_STAGED, variant, 32, 128, p.K) : route_of(DCCN_FAMILY_STAGED, variant, 64, 64, p.K);
    if (variant >= 1 && variant <= kCconvFwd16Rows && vec_both(p) && big < 2 * kCUs && kin % 2 == 0)
        return route16(DCCN_FAMILY_GEMM16, variant, kCconvFwd16[variant]);
    return route_generic<OP_KCONTIG, OP_CCONV_W>(p);
}
int cconv_fwd_impl(const float* x, const float* w, const float* bias, float* out, int rows, int kin, int F,
                          hipStream_t s, int ldx) {
    if (!x || !w || !out || rows <= 0 || kin <= 0 || F <= 0) return DCCN_ERR_INVALID_ARG;
    const GemmParams p = cconv_fwd_params(x, w, bias, out, rows, kin, F, ldx);
    const Route r = cconv_fwd_route(p, kin);
    if (r.family == DCCN_FAMILY_STAGED) switch (r.variant) {
        case 7: return launch_cconv_fwd_staged<8>(p, s);
        case 8: return launch_cconv_fwd_staged<4>(p, s);
        case 9: return launch_cconv_fwd_staged<10>(p, s);
        case 10: return launch_cconv_fwd_staged<8, 32, 128>(p, s);
        default: return launch_cconv_fwd_staged<4, 32, 128>(p, s);
    }
    if (r.family == DCCN_FAMILY_GEMM16) return kCconvFwd16Launch[r.variant](p, s);
    return launch_gemm<OP_KCONTIG, OP_CCONV_W, 0, TAG_CCONV_FWD>(p, 1, s);
}

int cconv_bwd_x_impl(const float* dout, const float* w, float* dx, int rows, int kin, int F, hipStream_t s,
                            int ldc) {
    if (!dout || !w || !dx || rows <= 0 || kin <= 0 || F <= 0) return DCCN_ERR_INVALID_ARG;
    return launch_gemm<OP_KCONTIG, OP_CCONV_WT, 0, TAG_CCONV_BWD_X>(cconv_bwd_x_params(dout, w, dx, rows, kin, F, ldc), 1, s);
}

// C-Conv fold and the tail's slab reduction in one launch: both are tiny, and the reduction has no consumer
// before the optimizer, so it rides on the fold instead of sitting on the critical path after the tail kernel
__global__ __launch_bounds__(256) void cconv_fold_finalize_kernel(const float* __restrict__ partial, int splits,
                                                                  long long slab, const float* __restrict__ colsum,
                                                                  float* __restrict__ dw, float* __restrict__ dbias,
                                                                  int kin, int F, int fold_blocks, TailFinalizeArgs a) {
    if ((int)blockIdx.x < fold_blocks) {
        cconv_fold_body(partial, splits, slab, colsum, dw, dbias, kin, F, blockIdx.x);
    } else {
        demod_tail_finalize_body(a, (int)blockIdx.x - fold_blocks);
    }
}

// the split-K C-Conv weight-gradient GEMM with the tail's slab reduction riding on extra blocks of the same launch
template <bool VEC, int BK = 64, int NBUF = 2>
__global__ __launch_bounds__(kGemmThreads) void cconv_bwd_w_finalize_kernel(const GemmParams p, int tiles, int gemm_blocks,
                                                                            TailFinalizeArgs a) {
    const int b = (int)blockIdx.x;
    stamp_mark(p.stamp, 0);
    if (b < gemm_blocks) {
        gemm_block<OP_ICONTIG, OP_ICONTIG, 64, 64, BK, 1, VEC, NBUF>(p, b % tiles, tiles, b / tiles);
    } else {
        demod_tail_finalize_body(a, b - gemm_blocks);
    }
    stamp_mark(p.stamp, 1);
}

// the same with the GEMM blocks in the k-major form (gemm_kmajor.h)
template <int BK>
__global__ __launch_bounds__(kGemmThreads) void cconv_bwd_w_km_finalize_kernel(const GemmParams p, int tiles, int gemm_blocks,
                                                                               TailFinalizeArgs a) {
    const int b = (int)blockIdx.x;
    stamp_mark(p.stamp, 0);
    if (b < gemm_blocks) {
        kmajor_block<1, BK>(p, b % tiles, tiles, b / tiles);
    } else {
        demod_tail_finalize_body(a, b - gemm_blocks);
    }
    stamp_mark(p.stamp, 1);
}

constexpr int kCconvBwMaxSplits = 128;
// TUNE_CCONV_BWD_W 1-4: gemm16 tiles of the C-Conv weight gradient
constexpr int kCconvBw16Rows = 4;
constexpr Tile16Cfg kCconvBw16[kCconvBw16Rows + 1] = {{},
    {2, 2, 2, 2, 32, 1},      // 64x64
    {2, 2, 1, 2, 32, 1},      // 32x64
    {1, 4, 5, 2, 32, 1},      // 80x128
    {2, 2, 1, 4, 32, 1}};     // 32x128
template <int V>
static int cconv_bw16_launch(const GemmParams& p, int splits, const TailFinalizeArgs& fin, hipStream_t s) {
    constexpr Tile16Cfg c = kCconvBw16[V];
    return launch_bwd_w16_finalize<c.wgm, c.wgn, c.tm, c.tn, c.bk>(p, splits, fin, s);
}
constexpr int (*kCconvBw16Launch[5])(const GemmParams&, int, const TailFinalizeArgs&, hipStream_t) = {nullptr,
    cconv_bw16_launch<1>, cconv_bw16_launch<2>, cconv_bw16_launch<3>, cconv_bw16_launch<4>};
// slab capacity of the C-Conv weight gradient: the legacy split plan, and at least kCconvBwMaxSplits slabs of a small output
static int cconv_bw_capacity(int rows, int kin, int F) {
    const int legacy = splitk_capacity(2 * kin, 2 * F, rows);
    return (4LL * kin * F > 512 * 512 || legacy > kCconvBwMaxSplits) ? legacy : kCconvBwMaxSplits;
}
size_t cconv_bw_ws_bytes(int rows, int kin, int F) {
    SlabWs w;
    return carved_bytes([&](Carver& c) { slab_carve(c, cconv_bw_capacity(rows, kin, F), 2 * kin, 2 * F, &w); });
}

// p.C = where the slabs will lie.  in_step: the training step's form -- the tail's slab reduction rides on the launch and the
// optimizer launch folds the slabs; only it takes the gemm16 rows and the split count of knob 5.
static int cconv_bwd_w_route(const GemmParams& p, int rows, int kin, int F, bool in_step, Route* out) {
    const int variant = g_tune[TUNE_CCONV_BWD_W] == kVariantKmajor ? 0 : g_tune[TUNE_CCONV_BWD_W];
    const bool small = 4LL * kin * F <= 512 * 512;
    const bool v16 = variant > 0 && in_step && vec_both(p) && small;
    if (v16) {
        if (variant > kCconvBw16Rows) return DCCN_ERR_INVALID_ARG;       // (no such row)
        int want = g_tune[TUNE_CCONV_BWD_SPLITS];
        const Tile16Cfg c16 = kCconvBw16[variant];
        const int tiles = ceil_div(2 * kin, c16.rows()) * ceil_div(2 * F, c16.cols());
        if (want <= 0) want = (2 * kCUs + tiles - 1) / tiles;
        if (want > kCconvBwMaxSplits) want = kCconvBwMaxSplits;
        *out = with_split(route16(DCCN_FAMILY_GEMM16, variant, c16), plan_splitk_n(rows, want, c16.bk));
        return DCCN_OK;
    }
    SplitPlan sp = plan_splitk(2 * kin, 2 * F, rows);
    if (g_tune[TUNE_CCONV_BWD_SPLITS] > 0 && in_step && small) {
        const int want = g_tune[TUNE_CCONV_BWD_SPLITS];
        sp = plan_splitk_n(rows, want < kCconvBwMaxSplits ? want : kCconvBwMaxSplits, 64);
    }
    // (large outputs, e.g. N = 1024: the 32x32x2 form measured 0.7 % faster per step -- the k-major form pays off where
    // the k-loops are short)
    const bool km = g_tune[TUNE_CCONV_BWD_W] == kVariantKmajor && kmajor_ok(p) && ceil_div(p.N, 64) * ceil_div(p.M, 64) <= 2 * kCUs;
    if (km) *out = with_split(route_of(DCCN_FAMILY_KMAJOR, 0, 64, 64, 64), sp);
    // the step's own launch of the 32x32x2 family: 128 rows per split run as one k-tile
    else if (in_step && vec_both(p)) *out = with_split(route_of(DCCN_FAMILY_GENERIC, 0, 64, 64, (sp.klen == 128 && g_whole_k) ? 128 : 64), sp);
    else {
        GemmParams q = p;
        q.klen = sp.klen;
        *out = route_generic<OP_ICONTIG, OP_ICONTIG>(q, sp.splits);
    }
    return DCCN_OK;
}

int cconv_bwd_w_impl(const float* x, const float* dout, float* dw, float* dbias, int rows, int kin, int F,
                            void* ws, size_t ws_bytes, hipStream_t s, const TailFinalizeArgs* fin,
                            FoldDefer* defer) {
    if (!x || !dout || !dw || rows <= 0 || kin <= 0 || F <= 0) return DCCN_ERR_INVALID_ARG;
    if (!ws || ws_bytes < cconv_bw_ws_bytes(rows, kin, F)) return DCCN_ERR_WORKSPACE;
    GemmParams p = cconv_bwd_w_params(x, dout, rows, kin, F);
    const bool in_step = defer && fin;
    p.C = static_cast<float*>(ws);                  // (slab_carve's first piece lies at the head of the workspace)
    Route r;
    DCCN_TRY(cconv_bwd_w_route(p, rows, kin, F, in_step, &r));
    const SplitPlan sp{r.splits, r.klen};
    Carver c(ws, ws_bytes);
    SlabWs sw;
    if (!slab_carve(c, sp.splits, 2 * kin, 2 * F, &sw)) return DCCN_ERR_WORKSPACE;
    float *slabs = sw.slabs, *cs = sw.colsum;
    p.C = slabs; p.colsum = cs;
    p.klen = sp.klen;
    if (r.family == DCCN_FAMILY_GEMM16) {
        DCCN_TRY(kCconvBw16Launch[r.variant](p, sp.splits, *fin, s));
        *defer = fold_defer(sw);
        return DCCN_OK;
    }
    if (in_step && vec_both(p)) {
        // fused step: GEMM + tail finalize in one launch; the fold happens inside the optimizer kernel
        const int tiles = ceil_div(p.N, 64) * ceil_div(p.M, 64), gemm_blocks = tiles * sp.splits;
        const dim3 grid(gemm_blocks + tail_finalize_blocks(fin->P));
        if (r.family == DCCN_FAMILY_KMAJOR) {
            auto kern = cconv_bwd_w_km_finalize_kernel<64>;
            constexpr size_t smem = kmajor_smem_bytes<64>();
            DCCN_TRY(set_max_dynamic_smem(reinterpret_cast<const void*>(kern), smem));
            hipLaunchKernelGGL(kern, grid, dim3(kGemmThreads), smem, s, p, tiles, gemm_blocks, *fin);
        } else if (r.tile_k == 128) {
            // 128 rows per split: the whole k range of a block as one tile (all loads in flight at once, no k-tile barrier)
            auto kern = cconv_bwd_w_finalize_kernel<true, 128, 1>;
            constexpr size_t smem = gemm_smem_bytes<OP_ICONTIG, OP_ICONTIG, 64, 64, 128, 1>();
            DCCN_TRY(set_max_dynamic_smem(reinterpret_cast<const void*>(kern), smem));
            hipLaunchKernelGGL(kern, grid, dim3(kGemmThreads), smem, s, p, tiles, gemm_blocks, *fin);
        } else {
            auto kern = cconv_bwd_w_finalize_kernel<true>;
            constexpr size_t smem = gemm_smem_bytes<OP_ICONTIG, OP_ICONTIG, 64, 64, 64>();
            DCCN_TRY(set_max_dynamic_smem(reinterpret_cast<const void*>(kern), smem));
            hipLaunchKernelGGL(kern, grid, dim3(kGemmThreads), smem, s, p, tiles, gemm_blocks, *fin);
        }
        DCCN_LAUNCH_CHECK();
        *defer = fold_defer(sw);
        return DCCN_OK;
    }
    if (defer) defer->slabs = nullptr;
    if (r.family == DCCN_FAMILY_KMAJOR)
        DCCN_TRY((launch_kmajor<1, TAG_CCONV_BWD_W>(p, sp.splits, s)));
    else
        DCCN_TRY((launch_gemm<OP_ICONTIG, OP_ICONTIG, 1, TAG_CCONV_BWD_W>(p, sp.splits, s)));
    if (defer && !fin) {                     // the caller's optimizer launch folds the slabs (eq_opt.h)
        *defer = fold_defer(sw);
        return DCCN_OK;
    }
    const int nthreads = kin * F + F;
    const int fold_blocks = ceil_div(nthreads, kRedLanes);
    if (fin)
        hipLaunchKernelGGL(cconv_fold_finalize_kernel, dim3(fold_blocks + tail_finalize_blocks(fin->P)), dim3(256), 0, s,
                           slabs, sp.splits, p.slab, cs, dw, dbias, kin, F, fold_blocks, *fin);
    else
        hipLaunchKernelGGL(cconv_fold_kernel, dim3(fold_blocks), dim3(256), 0, s, slabs, sp.splits, p.slab, cs, dw, dbias,
                           kin, F);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

// ---------------------------------------------------------------------------------------
// same-shaped C-Conv layers as grouped launches (the equaliser's corr / eq pair, model.py:439-449)
// ---------------------------------------------------------------------------------------
// forward of `groups` (1,kin)->F C-Convs: operands of group g at element strides gx / gw / gb from group 0.
// join_pairs: the two outputs are the IQ-pair streams of ONE [rows, F, 4] tensor (tf.concat on the last axis,
// model.py:456): out = that tensor, group g writes floats 2g, 2g+1 of every cell.  Returns false when the shapes do
// not qualify for the grouped kernels (the caller then runs the layers one by one).
bool cconv_pair_ok(const float* x, const float* w, const float* o, int rows, int kin, int F, long long gx, long long gw,
                          long long go) {
    return (kin % 2 == 0) && (F % 2 == 0) && (kin % 32 == 0) && (F % 32 == 0) && aligned16(x) && aligned16(w) && aligned16(o) &&
           (gx % 4 == 0) && (gw % 4 == 0) && (go % 2 == 0) && small_enough(rows, 4LL * (kin > F ? kin : F)) &&
           small_enough(kin, 2LL * F) && (long long)ceil_div(rows, 128) * ceil_div(2 * F, 128) < 2 * kCUs;
}
int cconv_fwd_grouped_impl(const float* x, const float* w, const float* bias, float* out, int rows, int kin, int F,
                                  int groups, long long gx, long long gw, long long gb, bool join_pairs, hipStream_t s) {
    if (!x || !w || !out || rows <= 0 || groups < 1 || groups > 2 || (join_pairs && groups != 2)) return DCCN_ERR_INVALID_ARG;
    // group 0's operands (cconv_pair_ok: the strides keep every group's as legal)
    const GemmParams p = cconv_fwd_params(x, w, bias, out, rows, kin, F, 0, join_pairs ? 4 * F : 0);
    if (!vec_both(p)) return DCCN_ERR_INVALID_ARG;
    GroupStride gs;
    gs.a = gx; gs.b = gw; gs.bias = gb; gs.colsum = 0;
    gs.c = join_pairs ? 2 : (long long)rows * 2 * F;
    if (join_pairs) {
        if (p.K == 128 && g_whole_k)
            return launch_gemm_grouped<OP_KCONTIG, OP_CCONV_W, 64, 64, 128, TAG_CCONV_FWD, 1, CMAP_JOIN_PAIRS>(p, gs, groups, s);
        return launch_gemm_grouped<OP_KCONTIG, OP_CCONV_W, 64, 64, 64, TAG_CCONV_FWD, 2, CMAP_JOIN_PAIRS>(p, gs, groups, s);
    }
    return launch_gemm_grouped<OP_KCONTIG, OP_CCONV_W, 64, 64, 64, TAG_CCONV_FWD, 2, CMAP_NONE>(p, gs, groups, s);
}

// backward of `groups` (1,kin)->F C-Convs in ONE launch: dx_g = dout_g . Weff_g^T and the split-K slabs of
// dWeff_g = x_g^T . dout_g (+ column sums), left un-folded in ws for the optimizer launch (defer[g]).
// Strides in elements: gx (x and dx), gd (dout), gw (kernels).
size_t cconv_bwd_grouped_ws_bytes(int rows, int kin, int F, int groups) {
    return (size_t)groups * cconv_bw_ws_bytes(rows, kin, F);
}
int cconv_bwd_grouped_impl(const float* x, const float* dout, const float* w, float* dx, int rows, int kin, int F,
                                  int groups, long long gx, long long gd, long long gw, void* ws, size_t ws_bytes,
                                  FoldDefer* defer, hipStream_t s) {
    if (!x || !dout || !w || !dx || !defer || rows <= 0 || groups < 1 || groups > 2) return DCCN_ERR_INVALID_ARG;
    if (!ws || ws_bytes < cconv_bwd_grouped_ws_bytes(rows, kin, F, groups)) return DCCN_ERR_WORKSPACE;
    SplitPlan sp = plan_splitk(2 * kin, 2 * F, rows);
    // (one output tile and > 16 384 rows: at most kCconvBwMaxSplits k ranges)
    if (sp.splits > kCconvBwMaxSplits) sp = plan_splitk_n(rows, kCconvBwMaxSplits, 64);
    if (sp.splits > kCconvBwMaxSplits) return DCCN_ERR_STATE;
    // group 0's share of the workspace; group g's lies `per` floats further
    const size_t per_bytes = cconv_bw_ws_bytes(rows, kin, F), per = per_bytes / sizeof(float);
    Carver c(ws, per_bytes);
    SlabWs sw;
    if (!slab_carve(c, sp.splits, 2 * kin, 2 * F, &sw)) return DCCN_ERR_WORKSPACE;
    const GemmParams px = cconv_bwd_x_params(dout, w, dx, rows, kin, F);
    GroupStride g1;
    g1.a = gd; g1.b = gw; g1.c = gx; g1.bias = 0; g1.colsum = 0;
    GemmParams pw = cconv_bwd_w_params(x, dout, rows, kin, F);
    pw.C = sw.slabs; pw.colsum = sw.colsum;
    pw.klen = sp.klen;
    if (!vec_both(px) || !vec_both(pw)) return DCCN_ERR_INVALID_ARG;
    if (!kmajor_ok(pw)) return DCCN_ERR_STATE;
    GroupStride g2;
    g2.a = gx; g2.b = gd; g2.c = (long long)per; g2.bias = 0; g2.colsum = (long long)per;
    DCCN_TRY(launch_cconv_bwd_grouped_km<64>(px, g1, pw, g2, sp.splits, groups, s));
    for (int g = 0; g < groups; ++g) {
        defer[g] = fold_defer(sw);
        defer[g].slabs += (size_t)g * per; defer[g].colsum += (size_t)g * per;
    }
    return DCCN_OK;
}

// ---------------------------------------------------------------------------------------
// backward of the basic receiver's training step in one launch (rx_bwd.h)
// ---------------------------------------------------------------------------------------
static int rx_bwd_fused_tiles(int batch, int S, int F) { return ceil_div(batch, 64) * ceil_div(S * 2 * F, 64); }
struct RxBwdWs { float *partial, *colsum; };     // dWeff partials, folded per dX tile: [kin][32][{a, b}] (rx_bwd.h); column sums
static RxBwdWs rx_bwd_fused_carve(Carver& c, int batch, int S, int kin, int F) {
    const size_t tiles = (size_t)rx_bwd_fused_tiles(batch, S, F);
    float* partial = c.take<float>(tiles * kin * 64);
    return RxBwdWs{partial, c.take<float>(tiles * 64)};
}
static size_t rx_bwd_fused_ws_bytes(int batch, int S, int kin, int F) {
    return carved_bytes([&](Carver& c) { rx_bwd_fused_carve(c, batch, S, kin, F); });
}
// applicable: 64x64 dX tiles that lie inside one symbol's 2F columns, 2kin = 128 or 160 (N = 64 without / with the
// cyclic prefix), the grouped k-major plan for the dense gradients, vector-legal operands
static bool rx_bwd_fused_ok(int batch, int S, int kin, int F, int D, const float* x_norm, const float* fft_out,
                            const float* dz, const float* wd) {
    const int dK = S * 2 * F, dN = 2 * D;
    if (!g_tune[TUNE_FUSED_BWD] || g_tune[TUNE_DENSE_BWD] != kVariantKmajor) return false;
    if ((2 * F) % 64 != 0 || (2 * kin != 128 && 2 * kin != 160)) return false;
    if (dN % 4 != 0 || !aligned16(x_norm) || !aligned16(fft_out) || !aligned16(dz) || !aligned16(wd)) return false;
    // (batch x dN: dz, the dW items' B operand -- a short, very wide dense layer under a long batch can pass every test below)
    if (!small_enough(batch, (long long)S * 2 * kin) || !small_enough(batch, dK) || !small_enough(dK, dN) ||
        !small_enough(batch, dN))
        return false;
    const long long big = (long long)ceil_div(batch, 128) * ceil_div(dK, 128);
    if (big >= 2 * kCUs) return false;
    const SplitPlan sp = dense_dw_plan(batch, dK, dN, kFusedBwdRangeRows);
    return (long long)ceil_div(dK, 128) * ceil_div(dN, 128) * sp.splits < 2 * kCUs;
}

// the dense dW items of the fused backward launch: pw as dense_bwd_w_params builds it, pw.C = where the slabs will lie.
// route.splits = the slabs the launch writes; route.klen = the uniform plan's range length (what the items use unless
// route.nranges > 0: then the graded ranges koff[0 .. nranges] of knob 14)
static int rx_bwd_route(const GemmParams& pw, int batch, int dK, int dN, Route* out) {
    if (!kmajor_ok(pw)) return DCCN_ERR_INVALID_ARG;
    const SplitPlan sp = dense_dw_plan(batch, dK, dN, kFusedBwdRangeRows);
    Route r = with_split(route_of(DCCN_FAMILY_RX_FUSED, 0, 64, 64, 64), sp);
    r.w_tile_rows = r.w_tile_cols = 64;
    if (g_tune[TUNE_DW_GRADED] > 0 && sp.splits > 1 && batch >= 768) {        // (>= 12 k-tiles: else the last ranges get too short)
        int off[9];
        const int n = graded_ranges(g_tune[TUNE_DW_GRADED], batch, off);
        if (n > 1 && n <= max_splits16(dK, dN)) {
            r.nranges = n; r.splits = n;
            memcpy(r.koff, off, sizeof(int) * (n + 1));
        }
    }
    *out = r;
    return DCCN_OK;
}

// dfft nullable: the dX tiles then only feed their epilogue
static int rx_bwd_fused_impl(const float* x_norm, const float* fft_out, const float* dz, const float* wd, float* dfft,
                             float* dbias_dense, int batch, int S, int kin, int F, int D, void* ws_dense, size_t ws_dense_bytes,
                             void* ws_conv, size_t ws_conv_bytes, const NormRideArgs& nr, const TailFinalizeArgs& fin,
                             dccn_adam_hparams hp, hipStream_t s, DeferredSlabs* ds, FoldDefer* fd, int* fold_tilew) {
    const int dK = S * 2 * F, dN = 2 * D;
    if (!ws_dense || ws_dense_bytes < splitk_ws_bytes(dK, dN, batch)) return DCCN_ERR_WORKSPACE;
    if (!ws_conv || ws_conv_bytes < rx_bwd_fused_ws_bytes(batch, S, kin, F)) return DCCN_ERR_WORKSPACE;
    GemmParams px = dense_bwd_x_params(dz, wd, dfft, batch, dK, dN);
    GemmParams pw = dense_bwd_w_params(fft_out, dz, batch, dK, dN);
    Route r;
    pw.C = static_cast<float*>(ws_dense);           // (slab_carve's first piece lies at the head of the workspace)
    DCCN_TRY(rx_bwd_route(pw, batch, dK, dN, &r));
    pw.klen = r.klen;
    const int nsplit = r.splits;
    if (r.nranges > 0) {
        pw.nranges = r.nranges;
        memcpy(pw.koff, r.koff, sizeof(pw.koff));
    }
    Carver c(ws_dense, ws_dense_bytes);
    SlabWs sw;
    if (!slab_carve(c, nsplit, dK, dN, &sw)) return DCCN_ERR_WORKSPACE;
    pw.C = sw.slabs; pw.colsum = dbias_dense ? sw.colsum : nullptr;
    Carver cc(ws_conv, ws_conv_bytes);
    const RxBwdWs cw = rx_bwd_fused_carve(cc, batch, S, kin, F);
    DweffArgs de;
    de.xn = x_norm; de.partial = cw.partial; de.colsum = cw.colsum;
    de.batch = batch; de.ldx = S * 2 * kin; de.two_kin = 2 * kin; de.two_F = 2 * F;
    de.prio = g_tune[TUNE_BWD_PRIO];
    if (2 * kin == 160) DCCN_TRY(launch_rx_bwd_fused<5>(px, pw, de, nsplit, nr, fin, hp, s));
    else DCCN_TRY(launch_rx_bwd_fused<4>(px, pw, de, nsplit, nr, fin, hp, s));
    *ds = deferred_slabs(sw, dbias_dense != nullptr, true);
    fd->slabs = cw.partial; fd->colsum = cw.colsum;
    fd->splits = ceil_div(batch, 64) * S;                       // terms per element: (row tile, symbol)
    fd->slab = (long long)((2 * F) / 64) * kin * 64;            // distance between consecutive terms (tiles folded: [kin][32][2])
    *fold_tilew = 64;
    return DCCN_OK;
}

// ---------------------------------------------------------------------------------------
// tail
// ---------------------------------------------------------------------------------------
static int tail_blocks(long long cells, bool quad4 = false) {
    // quad4 (nbits = 4 training): four lanes per cell, 194 VGPRs -> two blocks per CU
    long long b = ceil_div_ll(quad4 ? 4 * cells : cells, kTailThreads);
    const long long cap = quad4 ? kTailBlocksMax : kTailBlocks;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}
// per-block metrics and tail-gradient slabs of `nblocks` blocks (the tail's own launch, or the tiles of the fused dense + tail)
struct TailWs { TailBlockMetrics* blk_metrics; float* blk_grads; };
static TailWs tail_carve(Carver& c, size_t nblocks, int nbits) {
    TailBlockMetrics* bm = c.take<TailBlockMetrics>(nblocks);
    return TailWs{bm, c.take<float>(nblocks * tail_param_count(nbits))};
}
size_t tail_ws_bytes(long long cells, int nbits) {
    (void)cells;
    return carved_bytes([&](Carver& c) { tail_carve(c, kTailBlocksMax, nbits); });
}
// the slab reduction's arguments for the `nblocks` blocks a tail launch ran.  pp / power_out: optional R8 finish riding on it
static TailFinalizeArgs tail_finalize_args(const TailWs& w, int nblocks, bool bwd, int nbits, long long cells, dccn_metrics* metrics,
                                           float* dtailp, const PowerPartials* pp, float* power_out) {
    const bool pw = pp != nullptr && power_out != nullptr;
    TailFinalizeArgs fa{};          // (no optimizer bookkeeping, hand-off words or monitors: the fused steps add theirs)
    fa.blk_metrics = w.blk_metrics; fa.blk_grads = bwd ? w.blk_grads : nullptr; fa.nblocks = nblocks;
    fa.P = bwd ? tail_param_count(nbits) : 0; fa.count = cells * nbits;
    fa.metrics = metrics; fa.dtailp = bwd ? dtailp : nullptr; fa.power_partial = pw ? pp->partial : nullptr;
    fa.n_power = pw ? pp->n : 0; fa.power_denom = pw ? pp->denom : 1.0; fa.power_out = pw ? power_out : nullptr;
    return fa;
}
// defer != nullptr: do not launch the slab reduction; hand its arguments to the caller (fused steps)
static int tail_finish(const TailFinalizeArgs& fa, TailFinalizeArgs* defer, hipStream_t s) {
    if (defer) {
        *defer = fa;
        return DCCN_OK;
    }
    hipLaunchKernelGGL(demod_tail_finalize_kernel, dim3(tail_finalize_blocks(fa.P)), dim3(256), 0, s, fa);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

// the tail's own launch.  16-QAM training runs four lanes per cell (tail.h): 50 accumulators per lane, not 200
template <int NB>
static int tail_launch(bool bwd, const float* z, const int32_t* bits, const float* tailp, float* prob, float* dz,
                       long long cells, int nblk, TailBlockMetrics* bm, float* bg, unsigned long long* stamp, hipStream_t s) {
    if (bwd && NB == 4 && prob)
        DCCN_LAUNCH_CHAINS_Z(demod_tail_quad4_kernel<true>, dim3(nblk), dim3(kTailThreads), 0, s, z, bits, tailp, prob, dz,
                             cells, bm, bg, stamp);
    else if (bwd && NB == 4)
        DCCN_LAUNCH_CHAINS_Z(demod_tail_quad4_kernel<false>, dim3(nblk), dim3(kTailThreads), 0, s, z, bits, tailp, prob, dz,
                             cells, bm, bg, stamp);
    else if (bwd)
        DCCN_LAUNCH_CHAINS_Z((demod_tail_kernel<NB, true>), dim3(nblk), dim3(kTailThreads), 0, s, z, bits, tailp, prob,
                             dz, cells, bm, bg, stamp);
    else
        DCCN_LAUNCH_CHAINS_Z((demod_tail_kernel<NB, false>), dim3(nblk), dim3(kTailThreads), 0, s, z, bits, tailp, prob,
                             dz, cells, bm, bg, stamp);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

// pp / power_out, defer: as tail_finalize_args / tail_finish
int tail_impl(bool bwd, const float* z, const int32_t* bits, const float* tailp, float* prob,
                     dccn_metrics* metrics, float* dz, float* dtailp, long long cells, int nbits,
                     const PowerPartials* pp, float* power_out, void* ws, size_t ws_bytes, hipStream_t s,
                     TailFinalizeArgs* defer) {
    if (!z || !bits || !tailp || !metrics || cells <= 0 || nbits < 1 || nbits > 4) return DCCN_ERR_INVALID_ARG;
    if (bwd && (!dz || !dtailp)) return DCCN_ERR_INVALID_ARG;
    if (!ws || ws_bytes < tail_ws_bytes(cells, nbits)) return DCCN_ERR_WORKSPACE;
    Carver c(ws, ws_bytes);
    const TailWs tw = tail_carve(c, kTailBlocksMax, nbits);
    TailBlockMetrics* bm = tw.blk_metrics; float* bg = tw.blk_grads;
    const int nblk = tail_blocks(cells, bwd && nbits == 4);
    int st = DCCN_ERR_INVALID_ARG;
    switch (nbits) {
        case 1: st = tail_launch<1>(bwd, z, bits, tailp, prob, dz, cells, nblk, bm, bg, tl_stamp, s); break;
        case 2: st = tail_launch<2>(bwd, z, bits, tailp, prob, dz, cells, nblk, bm, bg, tl_stamp, s); break;
        case 3: st = tail_launch<3>(bwd, z, bits, tailp, prob, dz, cells, nblk, bm, bg, tl_stamp, s); break;
        case 4: st = tail_launch<4>(bwd, z, bits, tailp, prob, dz, cells, nblk, bm, bg, tl_stamp, s); break;
    }
    DCCN_TRY(st);
    if (!defer) DCCN_NO_CHAINS();
    return tail_finish(tail_finalize_args(tw, nblk, bwd, nbits, cells, metrics, dtailp, pp, power_out), defer, s);
}

// ---------------------------------------------------------------------------------------
// dense forward with the tail fused into its epilogue (gemm16.h EPI_TAIL: register layout for nbits <= 2, tile staged
// through LDS for nbits >= 3)
// ---------------------------------------------------------------------------------------
static int dense_tail_max_blocks(int M, int N) {
    const int b = ceil_div(M, 32) * ceil_div(N, 64);
    // few rows: the one-latency 16x16 tiles of fewrow.h carry the tail as well (one slab per tile)
    const int few = (M <= 96 && (N % 16) == 0) ? ceil_div(M, 16) * (N / 16) : 0;
    return few > b && few <= kTailBlocksMax ? few : b;
}
size_t dense_tail_ws_bytes(int M, int N, int nbits) {
    return carved_bytes([&](Carver& c) { tail_carve(c, (size_t)dense_tail_max_blocks(M, N), nbits); });
}
static bool dense_tail_shape_ok(int M, int K, int N, int nbits) {
    // nbits >= 3 (tail weights in LDS; nbits = 4 training in the quad-lane form): knob 13
    return g_tune[TUNE_DENSE_FWD] > 0 && nbits >= 1 && nbits <= 4 && M > 0 && K > 0 && N > 0 && (K % 4 == 0) && (N % 4 == 0) &&
           small_enough(M, K) && small_enough(K, N) && (long long)ceil_div(M, 128) * ceil_div(N, 128) < 2 * kCUs;
}
bool dense_tail_ok(const float* x, const float* w, int M, int K, int N, int nbits) {
    return dense_tail_shape_ok(M, K, N, nbits) && aligned16(x) && aligned16(w);
}
// which steps take the fused launch for 8-QAM / 16-QAM (knob 13: bit 0 = the lane-per-cell forms -- nbits 3, and nbits 4
// evaluation; bit 1 = the quad-lane form of 16-QAM training).  The operator dccn_dense_tail_* itself accepts every nbits.
// bit 2: BPSK / QPSK steps of LARGE layers (>= two rounds of 128x128 tiles) run the dense forward on the 128x128x32 tile
// family and the tail as its own launch.
bool dense_tail_planned(int nbits, bool train, int M, int N) {
    const int k = g_tune[TUNE_TAIL_FUSE_HI];
    if (nbits <= 2) return !((k & 4) && (long long)ceil_div(M, 128) * ceil_div(N, 128) >= 2 * kCUs);
    return (nbits == 4 && train) ? (k & 2) != 0 : (k & 1) != 0;
}

// The grid a fused dense forward runs, decided ONCE for dense_tail_impl and dense_decide_impl (nbits <= 2): both launch the
// same tiles over the same rows, so z -- and with it every decision -- has the bits the evaluation step computes
enum DenseGrid : int { DG_TILES = 0, DG_FEWROW, DG_RAGGED };
struct DenseRoute {
    DenseGrid grid;
    bool large;         // DG_TILES: 80x64 tiles, else 48x64
    int rag;            // DG_RAGGED: rows of the short last tile row
    int blocks;         // blocks of the launch (the tail writes one slab each)
};
static DenseRoute dense_tail_route(const GemmParams& p, int nbits) {
    const int M = p.M, N = p.N, ncol = ceil_div(N, 64);
    DenseRoute r{};
    // large layers (several rounds of 48x64 tiles): 80x64 tiles re-use the B tile for five row blocks instead of three
    // (C4: 1.42 -> 1.34 ms); the lane's ten cells go through the tail in two batches of five
    r.large = (long long)ceil_div(M, kDense48.rows()) * ncol >= 4LL * kCUs;
    // 80x64 tiles over a row count that leaves <= 32 rows for the last tile row (C4: 585 = 7 x 80 + 25): that row as 32x64 blocks
    constexpr int R = kDense80.rows();
    const int rag = (r.large && nbits <= 2 && g_tune[TUNE_DENSE_RAGGED] && M > R) ? M % R : 0;
    // few rows, BPSK / QPSK: every operand of a 16x16 tile requested at once, the tail on the tile's own registers (fewrow.h)
    const int few_tiles = ceil_div(M, 16) * (N / 16);
    const bool few = g_tune[TUNE_FEWROW] && g_tune[TUNE_SKINNY] > 0 && nbits <= 2 && M <= 96 && fewrow_ng_c(p, false) >= 10 &&
                     few_tiles <= kTailBlocksMax && few_tiles <= dense_tail_max_blocks(M, N);
    if (rag > 0 && rag <= kDense32.rows()) {
        r.grid = DG_RAGGED; r.rag = rag; r.blocks = ((M - rag) / R) * ncol + ncol;
    } else if (few) {
        r.grid = DG_FEWROW; r.blocks = few_tiles;
    } else {
        r.grid = DG_TILES; r.blocks = ceil_div(M, r.large ? R : kDense48.rows()) * ncol;
    }
    return r;
}
// the last `rag` rows of p as a description of their own (A and C advanced); p keeps the rows in front of them
static GemmParams split_last_rows(GemmParams& p, int rag) {
    GemmParams q = p;
    p.M -= rag;
    q.M = rag; q.A = p.A + (size_t)p.M * p.lda; q.C = p.C ? p.C + (size_t)p.M * p.ldc : nullptr;
    return q;
}

template <int NB, bool BWD>
static int dense_tail_launch(bool large, const GemmParams& p, const TailEpiParams& tp, hipStream_t s) {
    constexpr Tile16Cfg a = kDense48, b = kDense80;
    const size_t sm = tune_smem_min();
    if (large) return launch_dense_tail16<b.wgm, b.wgn, b.tm, b.tn, b.bk, b.ks, NB, BWD, 2>(p, tp, s, sm);
    return launch_dense_tail16<a.wgm, a.wgn, a.tm, a.tn, a.bk, a.ks, NB, BWD, 2>(p, tp, s, sm);
}

// z nullable (not materialised then).  defer: as tail_impl.
int dense_tail_impl(bool bwd, const float* x, const float* w, const float* bias, float* z, const int32_t* bits,
                           const float* tailp, float* prob, dccn_metrics* metrics, float* dz, float* dtailp, int M,
                           int K, int N, int nbits, const PowerPartials* pp, float* power_out, void* ws, size_t ws_bytes,
                           hipStream_t s, TailFinalizeArgs* defer) {
    if (!x || !w || !bits || !tailp || !metrics || M <= 0 || K <= 0 || N <= 0 || (N & 1) || nbits < 1 || nbits > 4)
        return DCCN_ERR_INVALID_ARG;
    if (bwd && (!dz || !dtailp)) return DCCN_ERR_INVALID_ARG;
    if (!dense_tail_ok(x, w, M, K, N, nbits)) return DCCN_ERR_INVALID_ARG;
    if (!ws || ws_bytes < dense_tail_ws_bytes(M, N, nbits)) return DCCN_ERR_WORKSPACE;
    const GemmParams p = dense_fwd_params(x, w, bias, z, M, K, N);
    if (!vec_both(p)) return DCCN_ERR_INVALID_ARG;          // (dense_tail_ok asks for exactly these)
    const DenseRoute r = dense_tail_route(p, nbits);
    Carver c(ws, ws_bytes);
    const TailWs tw = tail_carve(c, (size_t)dense_tail_max_blocks(M, N), nbits);
    const long long cells = (long long)M * (N / 2);
    TailEpiParams tp;
    tp.bits = bits; tp.tailp = tailp; tp.prob = prob; tp.dz = dz; tp.blk_metrics = tw.blk_metrics; tp.blk_grads = tw.blk_grads;
    tp.inv_count = 1.0f / (float)(cells * nbits);
    int st;
    if (r.grid == DG_RAGGED) {                      // (nbits <= 2)
        GemmParams p1 = p;
        const GemmParams p2 = split_last_rows(p1, r.rag);
        const int M1 = p1.M;
        TailEpiParams t2 = tp;
        t2.bits = tp.bits + (size_t)M1 * (N / 2) * nbits;
        t2.prob = tp.prob ? tp.prob + (size_t)M1 * (N / 2) * nbits * 2 : nullptr;
        t2.dz = tp.dz ? tp.dz + (size_t)M1 * N : nullptr;
        constexpr Tile16Cfg c80 = kDense80, c32 = kDense32;       // (the two-shape grid, as in dense_decide_impl)
        const size_t sm = tune_smem_min();
        if (nbits == 1) st = bwd ? launch_dense_tail16_ragged<c80.tm, c32.tm, c80.bk, 1, true, 2>(p1, tp, p2, t2, s, sm) : launch_dense_tail16_ragged<c80.tm, c32.tm, c80.bk, 1, false, 2>(p1, tp, p2, t2, s, sm);
        else st = bwd ? launch_dense_tail16_ragged<c80.tm, c32.tm, c80.bk, 2, true, 2>(p1, tp, p2, t2, s, sm) : launch_dense_tail16_ragged<c80.tm, c32.tm, c80.bk, 2, false, 2>(p1, tp, p2, t2, s, sm);
    } else if (r.grid == DG_FEWROW) {               // (nbits <= 2)
        if (nbits == 1) st = bwd ? launch_fewrow_tail<1, true>(p, tp, s) : launch_fewrow_tail<1, false>(p, tp, s);
        else st = bwd ? launch_fewrow_tail<2, true>(p, tp, s) : launch_fewrow_tail<2, false>(p, tp, s);
    }
    else if (nbits == 1) st = bwd ? dense_tail_launch<1, true>(r.large, p, tp, s) : dense_tail_launch<1, false>(r.large, p, tp, s);
    else if (nbits == 2) st = bwd ? dense_tail_launch<2, true>(r.large, p, tp, s) : dense_tail_launch<2, false>(r.large, p, tp, s);
    else if (nbits == 3) st = bwd ? dense_tail_launch<3, true>(r.large, p, tp, s) : dense_tail_launch<3, false>(r.large, p, tp, s);
    else st = bwd ? dense_tail_launch<4, true>(r.large, p, tp, s) : dense_tail_launch<4, false>(r.large, p, tp, s);
    DCCN_TRY(st);
    return tail_finish(tail_finalize_args(tw, r.blocks, bwd, nbits, cells, metrics, dtailp, pp, power_out), defer, s);
}

// ---------------------------------------------------------------------------------------
// receive path: the decision stage (decide.h) as its own launch and in the dense forward's epilogue
// ---------------------------------------------------------------------------------------
static int decide_row_bytes(int D, int nbits) { return (D * nbits + 7) / 8; }
// the decision stage stores a cell's llr as one vector (float2 at nbits = 2, float4 at nbits = 4) and prob as float2 pairs
bool decide_outputs_aligned(const float* llr, const float* prob, int nbits) {
    const uintptr_t la = nbits == 4 ? 15u : (nbits == 2 ? 7u : 3u);
    return (reinterpret_cast<uintptr_t>(llr) & la) == 0 && (reinterpret_cast<uintptr_t>(prob) & 7u) == 0;
}

int decide_impl(const float* z, const float* tailp, unsigned char* packed, float* llr, float* prob, int frames, int D,
                int nbits, hipStream_t s) {
    if (!z || !tailp || !packed || frames <= 0 || D <= 0 || nbits < 1 || nbits > 4) return DCCN_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(z) & 7u) != 0 || !decide_outputs_aligned(llr, prob, nbits)) return DCCN_ERR_INVALID_ARG;
    const int gpr = ceil_div(D, 8), RB = decide_row_bytes(D, nbits);
    const long long blocks = ceil_div_ll((long long)frames * gpr * 8, kDecideThreads);
    if (blocks > 0x7fffffffLL) return DCCN_ERR_INVALID_ARG;
    const dim3 grid((unsigned)blocks), blk(kDecideThreads);
    switch (nbits) {
        case 1: DCCN_LAUNCH_CHAINS_Z(demod_decide_kernel<1>, grid, blk, 0, s, z, tailp, packed, llr, prob, frames, D, gpr, RB); break;
        case 2: DCCN_LAUNCH_CHAINS_Z(demod_decide_kernel<2>, grid, blk, 0, s, z, tailp, packed, llr, prob, frames, D, gpr, RB); break;
        case 3: DCCN_LAUNCH_CHAINS_Z(demod_decide_kernel<3>, grid, blk, 0, s, z, tailp, packed, llr, prob, frames, D, gpr, RB); break;
        default: DCCN_LAUNCH_CHAINS_Z(demod_decide_kernel<4>, grid, blk, 0, s, z, tailp, packed, llr, prob, frames, D, gpr, RB); break;
    }
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

// Dense forward + decision on the grid dense_tail_route gives dense_tail_impl for the same operands (few-row tiles, 48x64,
// 80x64, the ragged two-shape grid).
// nbits <= 2: ONE launch, z nullable.  nbits >= 3: the 48x64 tiles store z (same k order as the LDS-staged tail of the fused
// evaluation launch), the stand-alone decision kernel follows; z must be given.
int dense_decide_impl(const float* x, const float* w, const float* bias, float* z, const float* tailp, unsigned char* packed,
                      float* llr, float* prob, int M, int K, int N, int nbits, hipStream_t s) {
    if (!x || !w || !tailp || !packed || M <= 0 || K <= 0 || N <= 0 || (N & 1) || nbits < 1 || nbits > 4)
        return DCCN_ERR_INVALID_ARG;
    if (!dense_tail_ok(x, w, M, K, N, nbits)) return DCCN_ERR_INVALID_ARG;
    if (nbits >= 3 && !z) return DCCN_ERR_INVALID_ARG;
    if (!decide_outputs_aligned(llr, prob, nbits)) return DCCN_ERR_INVALID_ARG;
    const GemmParams p = dense_fwd_params(x, w, bias, z, M, K, N);
    if (!vec_both(p)) return DCCN_ERR_INVALID_ARG;          // (dense_tail_ok asks for exactly these)
    const size_t sm = tune_smem_min();
    if (nbits >= 3) {
        DCCN_TRY(dense48_launch(p, s, sm));
        return decide_impl(z, tailp, packed, llr, prob, M, N / 2, nbits, s);
    }
    DecideEpiParams dq;
    dq.tailp = tailp; dq.packed = packed; dq.llr = llr; dq.prob = prob; dq.RB = decide_row_bytes(N / 2, nbits);
    const DenseRoute r = dense_tail_route(p, nbits);
    constexpr Tile16Cfg c48 = kDense48, c80 = kDense80, c32 = kDense32;
    if (r.grid == DG_RAGGED) {
        GemmParams p1 = p;
        const GemmParams p2 = split_last_rows(p1, r.rag);
        const int M1 = p1.M;
        DecideEpiParams d2 = dq;
        d2.packed = dq.packed + (size_t)M1 * dq.RB;
        d2.llr = dq.llr ? dq.llr + (size_t)M1 * (N / 2) * nbits : nullptr;
        d2.prob = dq.prob ? dq.prob + (size_t)M1 * (N / 2) * nbits * 2 : nullptr;
        return nbits == 1 ? launch_dense_decide16_ragged<c80.tm, c32.tm, c80.bk, 1, 2>(p1, dq, p2, d2, s, sm)
                          : launch_dense_decide16_ragged<c80.tm, c32.tm, c80.bk, 2, 2>(p1, dq, p2, d2, s, sm);
    }
    if (r.grid == DG_FEWROW) return nbits == 1 ? launch_fewrow_decide<1>(p, dq, s) : launch_fewrow_decide<2>(p, dq, s);
    if (r.large) return nbits == 1 ? launch_dense_decide16<c80.tm, c80.bk, 1, 2>(p, dq, s, sm) : launch_dense_decide16<c80.tm, c80.bk, 2, 2>(p, dq, s, sm);
    return nbits == 1 ? launch_dense_decide16<c48.tm, c48.bk, 1, 2>(p, dq, s, sm) : launch_dense_decide16<c48.tm, c48.bk, 2, 2>(p, dq, s, sm);
}

// prep = false: the per-step bookkeeping (alpha, beta powers, global_step) already rode on an earlier kernel of the step
int adam_impl(float* param, const float* grad, float* m, float* v, const float* reg_coef,
                     const float* reg_gate, dccn_adam_state* st, dccn_adam_hparams hp, long long n, hipStream_t s,
                     bool prep) {
    if (!param || !grad || !m || !v || !st || n <= 0) return DCCN_ERR_INVALID_ARG;
    if (prep) {
        hipLaunchKernelGGL(adam_prep_kernel, dim3(1), dim3(64), 0, s, st, hp);
        DCCN_LAUNCH_CHECK();
    }
    long long blocks = ceil_div_ll(ceil_div_ll(n, 4), 256);
    if (blocks > 4 * kCUs) blocks = 4 * kCUs;
    hipLaunchKernelGGL(adam_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, s, param, grad, m, v, reg_coef,
                       reg_gate, st, hp, n);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

// ---------------------------------------------------------------------------------------
// fused receiver step
// ---------------------------------------------------------------------------------------
static bool shape_ok(const dccn_rx_shape* sh) {
    return sh && sh->batch > 0 && sh->S > 0 && sh->kin > 0 && sh->F > 0 && sh->D > 0 && sh->nbits >= 1 &&
           sh->nbits <= 4;
}

RxLayout rx_layout(const dccn_rx_shape* sh) {
    RxLayout L;
    const long long F2 = 2LL * sh->F;
    L.o_conv_w = 0;
    L.o_conv_b = L.o_conv_w + (long long)sh->kin * F2;
    L.o_dense_w = L.o_conv_b + F2;
    L.o_dense_b = L.o_dense_w + (long long)sh->S * F2 * 2 * sh->D;
    L.o_tail = L.o_dense_b + 2LL * sh->D;
    L.total = L.o_tail + tail_param_count(sh->nbits);
    L.rows = sh->batch * sh->S;
    L.cols = sh->S * sh->kin * 2;
    L.dK = sh->S * sh->F * 2;
    L.dN = 2 * sh->D;
    L.cells = (long long)sh->batch * sh->D;
    L.ws_norm = norm_ws_bytes(sh->batch, L.cols);
    L.ws_tail = tail_ws_bytes(L.cells, sh->nbits);
    {
        const size_t f = dense_tail_ws_bytes(sh->batch, L.dN, sh->nbits);
        if (f > L.ws_tail) L.ws_tail = f;
    }
    L.ws_dense_bw = splitk_ws_bytes(L.dK, L.dN, sh->batch);
    L.ws_conv_bw = cconv_bw_ws_bytes(L.rows, sh->kin, sh->F);
    {
        const size_t f = rx_bwd_fused_ws_bytes(sh->batch, sh->S, sh->kin, sh->F);
        if (2LL * sh->kin <= 192 && f > L.ws_conv_bw) L.ws_conv_bw = f;
    }
    return L;
}
// the step's workspace: the regions of L.ws_* bytes its operators carve for themselves.  The receive step has R0's alone,
// an evaluation step also the tail's, a training step all four.
enum RxMode : int { RX_RECEIVE = 0, RX_EVAL, RX_TRAIN };
struct RxWs { void *norm, *tail, *dense_bw, *conv_bw; };
static RxWs rx_carve(Carver& c, const RxLayout& L, RxMode mode) {
    RxWs w{};
    w.norm = c.take<char>(L.ws_norm);
    if (mode >= RX_EVAL) w.tail = c.take<char>(L.ws_tail);
    if (mode == RX_TRAIN) {
        w.dense_bw = c.take<char>(L.ws_dense_bw);
        w.conv_bw = c.take<char>(L.ws_conv_bw);
    }
    return w;
}
static size_t rx_ws_bytes(const dccn_rx_shape* sh, RxMode mode) {
    const RxLayout L = rx_layout(sh);
    return carved_bytes([&](Carver& c) { rx_carve(c, L, mode); });
}

// The library's own second stream (one per device) and a pair of events per host thread: large layers run the dense kernel's
// optimizer update -- 3.2 GB of pure HBM traffic at N = 1024 -- NEXT TO the MFMA-bound C-Conv weight-gradient launch instead
// of behind it.  (Two kernels of one stream never overlap; blocks of two streams share the CUs.)
struct OverlapStreams {
    hipStream_t side;
    hipEvent_t fork, join;
};
static bool overlap_streams(OverlapStreams* o) {
    static std::mutex mu;
    static hipStream_t sides[64];
    thread_local hipEvent_t ev[64][2];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    {
        std::lock_guard<std::mutex> lock(mu);
        if (!sides[dev]) {
            // lowest priority: its own hardware queue (streams of one priority share a small pool of queues round-robin, and a
            // stream that lands on the main stream's queue does not overlap with it at all), and the MFMA-bound launch it
            // runs next to is served first whenever a CU has room
            int least = 0, greatest = 0;
            if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
            if (hipStreamCreateWithPriority(&sides[dev], hipStreamNonBlocking, least) != hipSuccess) { sides[dev] = nullptr; return false; }
        }
    }
    for (int k = 0; k < 2; ++k)
        if (!ev[dev][k] && hipEventCreateWithFlags(&ev[dev][k], hipEventDisableTiming) != hipSuccess) { ev[dev][k] = nullptr; return false; }
    o->side = sides[dev]; o->fork = ev[dev][0]; o->join = ev[dev][1];
    return true;
}

// ---- fused generator launch (datagen.h gen_static_frames_kernel / gen_doppler_frames_kernel; ABI entry points further down) ----
// does the descriptor's frame plan hold Doppler frames?  (doppler_period > 0 and a profile that is not the identity with
// Fd > 0.1: DeviceDataGen.frame_plan.)  Such a descriptor takes the Doppler instantiation of the launch.
bool gen_static_doppler(const dccn_gen_static* g) {
    if (!g || g->doppler_period <= 0) return false;
    if (g->n_profiles == 0) return !g->identity && g->Fd > 0.1f;
    for (int i = 0; i < g->n_profiles; ++i)
        if (!g->profiles[i].identity && g->profiles[i].Fd > 0.1f) return true;
    return false;
}
// the shapes the launch is instantiated for (dccn_gen_static_supported is this)
bool gen_static_shape_ok(int S, int K, int CP) { return S == 7 && K == 64 && (CP == 16 || CP == 4); }
static_assert(gen_static_smem_bytes<7, 64, 4>() == 18112, "short prefix: 16 x 132 grid floats + 2 x (476 + 128) samples");
bool gen_static_ok(const dccn_gen_static* g) {
    if (!g || !g->bits_out || !g->cell_map || !g->const_tab || !g->idft || !g->snr_db || !g->y || !g->noise || !g->power_partial)
        return false;
    if (g->frames <= 0 || g->frames > 65535 || g->S <= 0 || 2 * g->S > 16 || g->K <= 0 || g->CP < 0 || g->D <= 0 || g->nbits < 1 ||
        g->nbits > 4 || (g->n_profiles == 0 && (g->L <= 0 || g->L > 64)))
        return false;
    if (g->n_profiles < 0 || g->n_profiles > kGenMaxProfiles || (g->n_profiles > 0 && !g->profiles) || g->tap_stride < 0 ||
        (g->H_out && g->h_rep <= 0))
        return false;
    if (g->n_profiles == 0) {
        if (!g->identity && (!g->coeff || !g->alpha || g->n_taps <= 0 || g->n_taps > 16)) return false;
        if (g->tap_stride != 0 && g->tap_stride < g->n_taps) return false;
    }
    for (int i = 0; i < g->n_profiles; ++i) {
        const dccn_gen_profile& q = g->profiles[i];
        if (q.L <= 0 || q.L > 64) return false;
        if (!q.identity && (!q.coeff || !q.alpha || q.n_taps <= 0 || q.n_taps > 16 || g->tap_stride < q.n_taps)) return false;
    }
    // Doppler frames: a period, a symbol time and finite Doppler frequencies; a Doppler frame writes S distinct responses
    if (g->doppler_period < 0) return false;
    if (g->doppler_period > 0) {
        if (!(g->t_sym > 0.f) || !std::isfinite(g->t_sym)) return false;
        if (g->n_profiles == 0 && !std::isfinite(g->Fd)) return false;
        for (int i = 0; i < g->n_profiles; ++i)
            if (!std::isfinite(g->profiles[i].Fd)) return false;
        if (gen_static_doppler(g) && g->H_out && g->h_rep != g->S) return false;
    }
    // the instantiated shapes: the reference's N = 64 frame, 7 symbols x (64 + 16) samples at the long cyclic prefix and
    // 7 x (64 + 4) at the short one
    return gen_static_shape_ok(g->S, g->K, g->CP) && aligned16(g->y) && aligned16(g->noise);
}
// the generator launch's argument block from its descriptor (also used by launches that carry the generator's workgroups as
// riders: eq_step.h)
int gen_static_args(const dccn_gen_static* g, GenStaticArgs* out) {
    if (!gen_static_ok(g)) return DCCN_ERR_INVALID_ARG;
    if (ceil_div(g->frames, kGenFramesPerBlock) > kChanPartials) return DCCN_ERR_INVALID_ARG;
    GenStaticArgs& a = *out;
    a.bits_out = g->bits_out; a.cell_map = g->cell_map; a.const_tab = reinterpret_cast<const float2*>(g->const_tab);
    a.pilot = make_float2(g->pilot_re, g->pilot_im); a.idft = g->idft;
    memset(a.prof, 0, sizeof(a.prof));
    if (g->n_profiles == 0) {
        a.prof[0].coeff = g->coeff; a.prof[0].alpha = g->alpha; a.prof[0].n_taps = g->n_taps; a.prof[0].L = g->L;
        a.prof[0].identity = g->identity; a.prof[0].Fd = g->Fd;
        a.n_prof = 1;
        a.tap_stride = g->tap_stride > 0 ? g->tap_stride : g->n_taps;
    } else {
        for (int i = 0; i < g->n_profiles; ++i) {
            a.prof[i].coeff = g->profiles[i].coeff; a.prof[i].alpha = g->profiles[i].alpha;
            a.prof[i].n_taps = g->profiles[i].n_taps; a.prof[i].L = g->profiles[i].L; a.prof[i].identity = g->profiles[i].identity;
            a.prof[i].Fd = g->profiles[i].Fd;
        }
        a.n_prof = g->n_profiles;
        a.tap_stride = g->tap_stride;
    }
    a.H = reinterpret_cast<float2*>(g->H_out); a.h_rep = g->h_rep;
    a.dop_period = gen_static_doppler(g) ? g->doppler_period : 0; a.t_sym = g->t_sym;
    a.snr_db = g->snr_db; a.y = reinterpret_cast<float2*>(g->y); a.noise = reinterpret_cast<float2*>(g->noise);
    a.power_partial = g->power_partial; a.noise_partial = g->noise_partial; a.tx_out = g->tx_out;
    a.frames = g->frames; a.S = g->S; a.K = g->K; a.CP = g->CP; a.D = g->D; a.nbits = g->nbits;
    a.offset = g->offset; a.seed = g->seed;
#ifdef DCCN_ABLATION
    {
        static const int abl = getenv("DCCN_GEN_ABL") ? atoi(getenv("DCCN_GEN_ABL")) : 0;      // timing experiments only
        a.abl = abl;
    }
#else
    a.abl = 0;              // (the ablation switches of tools/genbench.py exist in `make ablation` builds only)
#endif
    return DCCN_OK;
}
int gen_static_launch(const dccn_gen_static* g, hipStream_t s, const GenChainScalars* chains) {
    GenStaticArgs a;
    DCCN_TRY(gen_static_args(g, &a));
    const int blocks = ceil_div(g->frames, kGenFramesPerBlock);
    GenChainScalars gc;
    if (chains) gc = *chains;
    else memset(&gc, 0, sizeof(gc));
    if (tl_chain.G > 1 && gc.n != tl_chain.G) return DCCN_ERR_UNSUPPORTED;      // (a group needs every chain's seed / offset)
    // (gen_static_ok: CP is 16 or 4)
    if (a.dop_period > 0) {       // (static descriptors keep the launch they had)
        if (g->CP == 16) {
            DCCN_LAUNCH_CHAINS_Z((gen_doppler_frames_kernel<7, 64, 16>), dim3(blocks), dim3(256), (gen_doppler_smem_bytes<7, 64, 16>()), s, a, gc);
        } else {
            DCCN_LAUNCH_CHAINS_Z((gen_doppler_frames_kernel<7, 64, 4>), dim3(blocks), dim3(256), (gen_doppler_smem_bytes<7, 64, 4>()), s, a, gc);
        }
    } else if (g->CP == 16) {
        DCCN_LAUNCH_CHAINS_Z((gen_static_frames_kernel<7, 64, 16>), dim3(blocks), dim3(256), (gen_static_smem_bytes<7, 64, 16>()), s, a, gc);
    } else {
        DCCN_LAUNCH_CHAINS_Z((gen_static_frames_kernel<7, 64, 4>), dim3(blocks), dim3(256), (gen_static_smem_bytes<7, 64, 4>()), s, a, gc);
    }
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

// ---- what a step launches for a shape: each condition is spelled ONCE.  The dccn_rx_* queries ask with null pointers
// ("given 16-byte aligned buffers"), the step's plan asks with the caller's buffers. ----
static bool rx_bwd_fused_ok(const dccn_rx_shape* sh, const float* x_norm, const float* fft_out, const float* dz, const float* wd) {
    return rx_bwd_fused_ok(sh->batch, sh->S, sh->kin, sh->F, sh->D, x_norm, fft_out, dz, wd);
}
// R2..R6 as one launch, the dense forward with the tail in its epilogue: z may be NULL
static bool rx_dense_tail_fused_ok(const dccn_rx_shape* sh, bool train, const float* fft_out, const float* wd) {
    return dense_tail_planned(sh->nbits, train, sh->batch, 2 * sh->D) &&
           dense_tail_ok(fft_out, wd, sh->batch, sh->S * 2 * sh->F, 2 * sh->D, sh->nbits);
}
// the receive step's dense forward + decision as ONE launch (then z may be NULL)
static bool rx_receive_fused(const dccn_rx_shape* sh, bool eval_tail_fused) {
    return sh->nbits <= 2 && eval_tail_fused;
}
// R0 of the next batch on the fused backward launch (fuse_bw), written to the second x_norm buffer
static bool rx_norm_rides_bwd_ok(const dccn_rx_shape* sh, bool fuse_bw, const float* x_next, const float* x_norm_next) {
    return g_tune[TUNE_NORM_ON_BWD] && fuse_bw && kNormFusedCG == 2 &&
           norm_fused_ok(x_next, x_norm_next, sh->batch, sh->S * sh->kin * 2);
}
// batches whose pipelined normalisation can read the fused generator's (y, noise, partials) as its input: the single-pass R0
// (norm_fused_kernel: <= 128 * kNormFusedRPT rows) and one power partial per generator block
static bool rx_gen_next_ok(const dccn_rx_shape* sh, const float* y, const float* x_norm) {
    return kNormFusedCG == 2 && ceil_div(sh->batch, kGenFramesPerBlock) <= kChanPartials &&
           norm_fused_ok(y, x_norm, sh->batch, sh->S * sh->kin * 2);
}

// R0 (+R8 partial sums into slot `slot`) of one batch as a step runs it; `ws_norm` is the carved region of L.ws_norm bytes
static int rx_norm_r0(const dccn_rx_shape* sh, const RxLayout& L, const float* x, float* y, bool want_power, PowerPartials* pp,
                      void* ws_norm, dccn_adam_hparams hp, int slot, hipStream_t s) {
    return norm_impl(x, y, nullptr, nullptr, want_power, pp, sh->batch, L.cols, 1e-9f, 8.0f, nullptr, hp, ws_norm, L.ws_norm, s, slot);
}

// Everything a step decides, decided before its first launch: rx_step_plan checks every argument and fills this, the
// rx_issue_* functions below only read it.  A refused step has launched nothing (also inside a stream capture).
struct RxStepPlan {
    RxLayout L;
    RxWs ws;
    bool train;
    bool pre;                       // x_norm already holds this batch (dccn_rx_buffers.x_prenormalised)
    int nslot;
    bool fused_tail;                // R2..R6 as one launch (z nullable)
    bool can_defer;                 // the optimizer launch takes over the C-Conv fold
    bool fuse_bw;                   // the backward as one launch (dfft nullable)
    bool ride_bw, ride_opt;         // R0 of the next batch on the backward / on the optimizer launch ...
    bool norm_after;                // ... or as launches of its own (shapes the single-pass kernel does not take)
    bool wait_x;                    // the launch that reads the next batch waits for the producer's event first
    const dccn_gen_static* gen;     // the next batch comes from the fused generator (gen_next)
    bool gen_window;                // ... read through the window behind the cyclic prefix (kin == K: a cp=False receiver)
    OverlapStreams branch;          // forked variant (dccn_rx_graph_create mode bit 1): dense dW/db on the caller's second stream
    bool want_overlap;              // large layers: the dense kernel's update on the library's second stream (ovs)
    OverlapStreams ovs;
};
// every return between a fork onto o->side and the join (a failed launch, a DCCN_TRY) still joins: the side stream never
// keeps running behind a call that has returned, and a capture of `s` is never left with an un-joined branch
struct OverlapJoin {
    const OverlapStreams* o; hipStream_t s; bool forked = false, joined = false;
    ~OverlapJoin() {
        if (forked && !joined) {
            (void)hipEventRecord(o->join, o->side);
            (void)hipStreamWaitEvent(s, o->join, 0);
        }
    }
};
// what one phase of the step leaves for the next
struct RxStepCarry {
    TailFinalizeArgs fin;
    DeferredSlabs ds;
    FoldDefer fd;
    int fold_tilew;
};

// launches nothing, records and waits on no event (overlap_streams only looks up what dccn_rx_workspace_size created)
static int rx_step_plan(const dccn_rx_shape* sh, const dccn_rx_buffers* b, bool train, const OverlapStreams* fork,
                        RxStepPlan* plan) {
    if (!b->x || !b->bits || !b->params || !b->x_norm || !b->fft_out || !b->metrics) return DCCN_ERR_INVALID_ARG;
    if (train && (!b->grads || !b->adam_m || !b->adam_v || !b->adam || !b->dz)) return DCCN_ERR_INVALID_ARG;
    if (!b->workspace || b->workspace_bytes < rx_ws_bytes(sh, train ? RX_TRAIN : RX_EVAL)) return DCCN_ERR_WORKSPACE;
    if (b->x_prenormalised != 0 && b->x_prenormalised != 1) return DCCN_ERR_INVALID_ARG;
    RxStepPlan& p = *plan;
    p = RxStepPlan{};
    const RxLayout& L = p.L = rx_layout(sh);
    Carver c(b->workspace, b->workspace_bytes);
    p.ws = rx_carve(c, L, train ? RX_TRAIN : RX_EVAL);
    const float* wd = b->params + L.o_dense_w;
    p.train = train;
    p.pre = train && b->x_prenormalised != 0;
    p.nslot = b->norm_slot ? 1 : 0;
    p.fused_tail = rx_dense_tail_fused_ok(sh, train, b->fft_out, wd);
    if (!p.fused_tail && !b->z) return DCCN_ERR_INVALID_ARG;            // ask dccn_rx_dense_tail_fused first
    if (!train) return DCCN_OK;

    const bool side = fork != nullptr;
    if (side) p.branch = *fork;
    p.can_defer = L.o_conv_w == 0 && (L.o_dense_w % 4) == 0;
    // small layers: dX tiles + C-Conv weight-gradient partials in their epilogue + dW items + tail finalize: one launch
    p.fuse_bw = !side && p.can_defer && rx_bwd_fused_ok(sh, b->x_norm, b->fft_out, b->dz, wd);
    if (!p.fuse_bw && !b->dfft) return DCCN_ERR_INVALID_ARG;            // ask dccn_rx_bwd_fused_supported first
    const bool second_buf = b->x_next != nullptr && b->x_norm_next != nullptr;
    p.ride_bw = second_buf && rx_norm_rides_bwd_ok(sh, p.fuse_bw, b->x_next, b->x_norm_next);
    if (second_buf && !p.ride_bw) return DCCN_ERR_INVALID_ARG;          // ask dccn_rx_norm_rides_backward first
    // gen_next: the generator launch of the NEXT batch is the step's first launch and the optimizer launch, its last one, reads
    // (y, noise, power partials) as R0's virtual input instead of a materialised x_next (x_next, when given too, receives x).
    // x_next_ready set as well: the caller has issued the generator itself on ANOTHER stream.  The double-buffered pipelining
    // has no virtual-input form: refuse rather than normalise a stale x_next (dccn_rx_gen_next_supported is the caller's query)
    // kin == K + CP: R0 reads the generator's whole symbols.  kin == K (a cp=False receiver, model.py:1236-1240): R0 reads the K
    // samples behind the cyclic prefix of every symbol (norm_adam.h NormVirtual, the windowed instantiation; x_next, when given,
    // receives that window).  Any other kin is refused.
    p.gen = b->gen_next;
    if (p.gen != nullptr) {
        const bool whole = sh->kin == p.gen->K + p.gen->CP, window = !whole && sh->kin == p.gen->K;
        if (p.gen->frames != sh->batch || p.gen->S != sh->S || !(whole || window)) return DCCN_ERR_INVALID_ARG;
        if (b->x_norm_next != nullptr || !gen_static_ok(p.gen) || !rx_gen_next_ok(sh, p.gen->y, b->x_norm))
            return DCCN_ERR_INVALID_ARG;
        // the source as the window reads it: rows of S * 2 (K + CP) floats, 2 K floats from 2 CP floats into each symbol -- whole
        // float4s, and the 2 K = 128 the windowed kernel is instantiated for
        if (window && (2 * p.gen->K != kWinK2 || (2 * p.gen->CP) % 4 != 0 ||
                       !norm_fused_ok(p.gen->y, b->x_norm, sh->batch, sh->S * 2 * (p.gen->K + p.gen->CP))))
            return DCCN_ERR_INVALID_ARG;
        p.gen_window = window;
    }
    const float* rin = p.gen ? p.gen->y : b->x_next;
    p.ride_opt = !p.ride_bw && rin != nullptr && kNormFusedCG == 2 && norm_fused_ok(rin, b->x_norm, sh->batch, L.cols);
    p.norm_after = b->x_next != nullptr && !p.ride_opt && !p.ride_bw;
    p.wait_x = rin != nullptr && b->x_next_ready != nullptr;
    // Large layers whose dW tiles are unsplit (N = 1024: 585 rows are one k range), grouped backward: the dense kernel's Adam
    // update runs as a launch of its own on the library's second stream next to the C-Conv weight-gradient launch
    if (!p.fuse_bw && !side && g_tune[TUNE_ADAM_OVERLAP] && p.can_defer && (((long long)L.dK * L.dN) % 4) == 0 &&
        (long long)ceil_div(L.dK, 128) * ceil_div(L.dN, 128) >= 2 * kCUs && dense_dw_plan(sh->batch, L.dK, L.dN).splits == 1)
        p.want_overlap = overlap_streams(&p.ovs);
    return DCCN_OK;
}

// step timeline (dccn_step_trace_enable): launch slots 1 C-Conv forward, 2 dense forward (+ tail), 3 tail (own launch),
// 4 backward (fused, or grouped dX+dW), 5 C-Conv weight gradient (own launch), 6 optimizer; 0 and 7 are never written.
// Launches issued while no slot is named carry no marks: R0, the generator of the next batch, the tail's slab reduction
// where it is a launch of its own (evaluation steps, the Adam-overlap plan) and whatever runs on a second stream.
static int rx_issue_forward(const dccn_rx_shape* sh, const dccn_rx_buffers* b, const RxStepPlan& p, dccn_adam_hparams hp,
                            hipStream_t s, const StepTraceScope& trace, TailFinalizeArgs* fin) {
    const RxLayout& L = p.L;
    const float* P = b->params;
    float* gtail = p.train ? b->grads + L.o_tail : nullptr;
    if (p.gen != nullptr && b->x_next_ready == nullptr) DCCN_TRY(gen_static_launch(p.gen, s));
    // R0 (+R8 partial sums) -- unless the previous call already normalised this batch behind its Adam update
    PowerPartials pp;
    if (p.pre) norm_power_partials(sh->batch, L.cols, p.ws.norm, L.ws_norm, b->x_next ? b->x_next : b->x, b->x_norm, &pp, p.nslot);
    else DCCN_TRY(rx_norm_r0(sh, L, b->x, b->x_norm, b->tx_power != nullptr, &pp, p.ws.norm, hp, p.nslot, s));
    // R1
    trace.launch(1);
    DCCN_TRY(cconv_fwd_impl(b->x_norm, P + L.o_conv_w, P + L.o_conv_b, b->fft_out, L.rows, sh->kin, sh->F, s));
    trace.launch(2);
    // R2 with R3-R6 (+ tail backward) in its epilogue; z is materialised only when the caller gave a buffer
    if (p.fused_tail)
        return dense_tail_impl(p.train, b->fft_out, P + L.o_dense_w, P + L.o_dense_b, b->z, b->bits, P + L.o_tail, b->prob,
                               b->metrics, b->dz, gtail, sh->batch, L.dK, L.dN, sh->nbits, &pp, b->tx_power, p.ws.tail,
                               L.ws_tail, s, p.train ? fin : nullptr);
    // R2, then R3-R6 (+ tail backward)
    DCCN_TRY(dense_fwd_impl(b->fft_out, P + L.o_dense_w, P + L.o_dense_b, b->z, sh->batch, L.dK, L.dN, s));
    trace.launch(3);
    return tail_impl(p.train, b->z, b->bits, P + L.o_tail, b->prob, b->metrics, b->dz, gtail, L.cells, sh->nbits, &pp,
                     b->tx_power, p.ws.tail, L.ws_tail, s, p.train ? fin : nullptr);
}

// the optimizer launch's argument block: what the main launch and the dense kernel's update on the second stream share
// (value-initialised: a field neither call site sets is zero on the device)
static AdamRxArgs adam_rx_args(const dccn_rx_buffers* b, const RxLayout& L) {
    AdamRxArgs a{};
    a.param = b->params; a.grad = b->grads; a.m = b->adam_m; a.v = b->adam_v;
    a.reg_coef = b->reg_coef; a.reg_gate = b->reg_coef ? &b->metrics->berlin : nullptr;
    a.state = b->adam;
    a.o_dw = L.o_dense_w; a.n_dw = (long long)L.dK * L.dN; a.o_db = L.o_dense_b; a.n_db = L.dN;
    a.neps = 1e-9f; a.npeak = 8.0f;
    a.reg_uniform_dw = b->reg_uniform_dense != 0 ? 1 : 0;
    return a;
}

static int rx_issue_backward(const dccn_rx_shape* sh, const dccn_rx_buffers* b, const RxStepPlan& p, dccn_adam_hparams hp,
                             hipStream_t s, RxStepCarry* k, OverlapJoin* ojoin) {
    const RxLayout& L = p.L;
    const float* wd = b->params + L.o_dense_w;
    float* G = b->grads;
    if (p.fuse_bw) {
        // R0 of the next batch: on leading (or closing) blocks of this launch when the caller gave the second x_norm buffer
        NormRideArgs nr{};
        if (p.ride_bw) {
            if (p.wait_x) DCCN_HIP(hipStreamWaitEvent(s, (hipEvent_t)b->x_next_ready, 0));
            PowerPartials np;
            norm_power_partials(sh->batch, L.cols, p.ws.norm, L.ws_norm, b->x_next, b->x_norm_next, &np, p.nslot ^ 1);
            nr.x = b->x_next; nr.y = b->x_norm_next; nr.power = b->tx_power ? const_cast<double*>(np.partial) : nullptr;
            nr.batch = sh->batch; nr.cols = L.cols; nr.blocks = norm_fused_blocks(L.cols);
            nr.eps = 1e-9f; nr.peak = 8.0f;
            nr.trail = g_tune[TUNE_NORM_ON_BWD] >= 2 ? 1 : 0;
        }
        return rx_bwd_fused_impl(b->x_norm, b->fft_out, b->dz, wd, b->dfft, G + L.o_dense_b, sh->batch, sh->S, sh->kin, sh->F,
                                 sh->D, p.ws.dense_bw, L.ws_dense_bw, p.ws.conv_bw, L.ws_conv_bw, nr, k->fin, hp, s, &k->ds, &k->fd,
                                 &k->fold_tilew);
    }
    if (p.branch.side) {
        // two-stream variant: dense dW/db on `side`, dX -> C-Conv dW on the main stream (joined in rx_issue_update)
        DCCN_HIP(hipEventRecord(p.branch.fork, s));
        DCCN_HIP(hipStreamWaitEvent(p.branch.side, p.branch.fork, 0));
        // (only a captured step forks, and a captured step carries no timeline stamps: both launches are unmarked)
        DCCN_TRY(dense_bwd_w_impl(b->fft_out, b->dz, G + L.o_dense_w, G + L.o_dense_b, sh->batch, L.dK, L.dN, p.ws.dense_bw,
                                  L.ws_dense_bw, p.branch.side, &k->ds));
        DCCN_HIP(hipEventRecord(p.branch.join, p.branch.side));
        return dense_bwd_x_impl(b->dz, wd, b->dfft, sh->batch, L.dK, L.dN, s);
    }
    // default: dense dX and dW/db in one grouped launch (independent GEMMs packed on the same grid)
    if (p.want_overlap) {
        // the update on the second stream needs this step's alpha and BER gate, so the tail's slab reduction (which otherwise
        // rides on the C-Conv weight-gradient launch) runs first, as a launch of its own
        hipLaunchKernelGGL(demod_tail_finalize_kernel, dim3(tail_finalize_blocks(k->fin.P)), dim3(256), 0, s, k->fin);
        DCCN_LAUNCH_CHECK();
        k->fin.metrics = nullptr;
    }
    DCCN_TRY(dense_bwd_grouped_impl(b->fft_out, b->dz, wd, b->dfft, G + L.o_dense_w, G + L.o_dense_b, sh->batch, L.dK, L.dN,
                                    p.ws.dense_bw, L.ws_dense_bw, s, &k->ds));
    // (the plan saw an unsplit dW; knobs 1 and 4 can make the grouped launch split a very wide, very short dense kernel
    // after all: its slabs are then summed by the main optimizer launch and nothing is forked)
    if (!p.want_overlap || k->ds.dw_slabs != nullptr) return DCCN_OK;
    // the optimizer kernel itself, restricted to the dense kernel's segment: same arithmetic, same results
    AdamRxArgs as = adam_rx_args(b, L);
    as.n = as.o_dw + as.n_dw;
    as.skip_hi = as.o_dw;                       // (everything in front of the dense kernel stays with the main launch)
    as.splits = 1;
    as.nt = g_tune[TUNE_ADAM_OVERLAP] >= 2 ? 2 : 0;
    long long sb = ceil_div_ll(ceil_div_ll(as.n, 4), 256);
    if (sb > 8 * kCUs) sb = 8 * kCUs;           // (2, 4, 16 per CU measured within 0.5 % of this)
    DCCN_HIP(hipEventRecord(p.ovs.fork, s));
    DCCN_HIP(hipStreamWaitEvent(p.ovs.side, p.ovs.fork, 0));
    ojoin->forked = true;
    hipLaunchKernelGGL(adam_rx_kernel<0>, dim3((unsigned)sb), dim3(256), 0, p.ovs.side, as, hp);
    DCCN_LAUNCH_CHECK();
    DCCN_HIP(hipEventRecord(p.ovs.join, p.ovs.side));
    return DCCN_OK;
}

// the optimizer launch: the instantiation for the dense gradient's split count (2..6, windowed 2..4; any other count takes
// the runtime form).  win: the windowed instantiation of R0 rides, a kernel of its own, launched by such steps only
static void launch_adam_rx(bool win, int splits, long long blocks, hipStream_t s, const AdamRxArgs& aa, const dccn_adam_hparams& hp) {
    void (*kern)(const AdamRxArgs, const dccn_adam_hparams) = win ? adam_rx_window_kernel<0> : adam_rx_kernel<0>;
    switch (splits) {
        case 2: kern = win ? adam_rx_window_kernel<2> : adam_rx_kernel<2>; break;
        case 3: kern = win ? adam_rx_window_kernel<3> : adam_rx_kernel<3>; break;
        case 4: kern = win ? adam_rx_window_kernel<4> : adam_rx_kernel<4>; break;
        case 5: if (!win) kern = adam_rx_kernel<5>; break;
        case 6: if (!win) kern = adam_rx_kernel<6>; break;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, s, aa, hp);
}
static int rx_issue_update(const dccn_rx_shape* sh, const dccn_rx_buffers* b, const RxStepPlan& p, dccn_adam_hparams hp,
                           hipStream_t s, const StepTraceScope& trace, RxStepCarry* k, OverlapJoin* ojoin) {
    const RxLayout& L = p.L;
    const FoldDefer& fd = k->fd;
    // C-Conv dW/db from dX (the C-Conv input is data: no dX of its own)
    // (its fold launch also carries the tail's slab reduction: metrics, tail gradients, tx_power)
    trace.launch(5);
    if (!p.fuse_bw)
        DCCN_TRY(cconv_bwd_w_impl(b->x_norm, b->dfft, b->grads + L.o_conv_w, b->grads + L.o_conv_b, L.rows, sh->kin, sh->F,
                                  p.ws.conv_bw, L.ws_conv_bw, s, &k->fin, p.can_defer ? &k->fd : nullptr));
    if (p.branch.side) DCCN_HIP(hipStreamWaitEvent(s, p.branch.join, 0));
    if (p.wait_x && !p.ride_bw) DCCN_HIP(hipStreamWaitEvent(s, (hipEvent_t)b->x_next_ready, 0));
    // R7 (+ BER-gated L2 term of R6), fused with the split-K reduction of the dense gradient and the C-Conv fold
    trace.launch(6);
    AdamRxArgs aa = adam_rx_args(b, L);
    aa.stamp = tl_stamp;
    aa.n = L.total;
    aa.dw_slabs = k->ds.dw_slabs; aa.db_slabs = k->ds.db_slabs; aa.splits = k->ds.splits;
    aa.kin = sh->kin; aa.F = sh->F; aa.o_cw = L.o_conv_w;
    aa.n_conv = L.o_dense_w;                      // C-Conv kernel + bias come first in the arena
    if (fd.slabs) {
        aa.cw_slabs = fd.slabs; aa.cw_colsum = fd.colsum; aa.cw_splits = fd.splits; aa.cw_slab = fd.slab;
        aa.cw_tilew = k->fold_tilew;
        aa.fold_blocks = ceil_div(sh->kin * sh->F + sh->F, k->fold_tilew > 0 ? kFoldLanesTiled : kRedLanes);
    }
    aa.skip_dw_grad = b->keep_dense_grad < 0 ? 1 : 0;          // the caller never reads the summed dense gradient
    // (the dense kernel's update forked onto the second stream is joined at the END of the call: this launch leaves that
    // segment alone and reads the same read-only step state)
    if (ojoin->forked) { aa.skip_lo = aa.o_dw; aa.skip_hi = aa.o_dw + aa.n_dw; }
    long long blocks = ceil_div_ll(ceil_div_ll(L.total - (aa.fold_blocks ? aa.n_conv : 0), 4), 256);
    if (blocks > 8 * kCUs) blocks = 8 * kCUs;
    blocks += aa.fold_blocks;
    aa.nv = norm_virtual_none();
    if (p.ride_opt) {
        // R0 of the next batch on the leading blocks of this launch (x_next, or gen_next's virtual input)
        const float* rin = p.gen ? p.gen->y : b->x_next;
        PowerPartials np;
        norm_power_partials(sh->batch, L.cols, p.ws.norm, L.ws_norm, rin, b->x_norm, &np, p.nslot);
        aa.nx = rin; aa.ny = b->x_norm; aa.npower = b->tx_power ? const_cast<double*>(np.partial) : nullptr;
        aa.nbatch = sh->batch; aa.ncols = L.cols; aa.norm_blocks = norm_fused_blocks(L.cols);
        blocks += aa.norm_blocks;
        const int npart = p.gen ? ceil_div(p.gen->frames, kGenFramesPerBlock) : 0;
        if (p.gen_window) aa.nv = norm_virtual_gen_window(p.gen, npart, const_cast<float*>(b->x_next));
        else if (p.gen) aa.nv = norm_virtual_gen(p.gen, npart, const_cast<float*>(b->x_next));
    }
    launch_adam_rx(p.ride_opt && p.gen_window, k->ds.splits, blocks, s, aa, hp);
    DCCN_LAUNCH_CHECK();
    trace.none();
    if (p.norm_after) {
        PowerPartials np;
        DCCN_TRY(rx_norm_r0(sh, L, b->x_next, b->x_norm, b->tx_power != nullptr, &np, p.ws.norm, hp, p.nslot, s));
    }
    if (ojoin->forked) { ojoin->joined = true; DCCN_HIP(hipStreamWaitEvent(s, p.ovs.join, 0)); }
    return DCCN_OK;
}

// fork != nullptr: run the dense weight-gradient branch on fork->side (fork/join by its events),
// concurrently with dX -> C-Conv weight gradient on the main stream.
static int rx_step_impl(const dccn_rx_shape* sh, const dccn_rx_buffers* b, bool train, dccn_adam_hparams hp,
                        hipStream_t s, const OverlapStreams* fork) {
    if (!shape_ok(sh) || !b) return DCCN_ERR_INVALID_ARG;
    const TuneScope tune(b->tuning);
    RxStepPlan plan;
    DCCN_TRY(rx_step_plan(sh, b, train, fork, &plan));
    const StepTraceScope trace;
    RxStepCarry k;
    k.fd.slabs = nullptr;
    k.fold_tilew = 0;
    DCCN_TRY(rx_issue_forward(sh, b, plan, hp, s, trace, &k.fin));
    if (!train) return DCCN_OK;
    trace.launch(4);
    k.fin.adam = b->adam;               // the optimizer's per-step bookkeeping rides on the tail finalize stage
    k.fin.hp = hp;
    OverlapJoin ojoin{&plan.ovs, s};
    DCCN_TRY(rx_issue_backward(sh, b, plan, hp, s, &k, &ojoin));
    return rx_issue_update(sh, b, plan, hp, s, trace, &k, &ojoin);
}

// ---------------------------------------------------------------------------------------
// receive step: R0 -> C-Conv forward -> dense + decision (no labels, no loss, no metrics)
// ---------------------------------------------------------------------------------------
static int rx_receive_impl(const dccn_rx_shape* sh, const dccn_rx_receive_buffers* b, hipStream_t s) {
    if (!shape_ok(sh) || !b) return DCCN_ERR_INVALID_ARG;
    const TuneScope tune(b->tuning);
    if (!b->x || !b->params || !b->x_norm || !b->fft_out || !b->packed) return DCCN_ERR_INVALID_ARG;
    if (!b->workspace || b->workspace_bytes < rx_ws_bytes(sh, RX_RECEIVE)) return DCCN_ERR_WORKSPACE;
    const RxLayout L = rx_layout(sh);
    const float* P = b->params;
    // the dense forward runs the plan the evaluation step would take for this shape (same bits in z)
    const bool via_tail_plan = rx_dense_tail_fused_ok(sh, false, b->fft_out, P + L.o_dense_w);
    const bool one_launch = rx_receive_fused(sh, via_tail_plan);
    if (!b->z && !one_launch) return DCCN_ERR_INVALID_ARG;
    // what dense_decide_impl / decide_impl ask of the buffers (the stand-alone decision kernel reads z as float2), asked
    // before the first launch
    if (!decide_outputs_aligned(b->llr, b->prob, sh->nbits) || (!one_launch && (reinterpret_cast<uintptr_t>(b->z) & 7u) != 0))
        return DCCN_ERR_INVALID_ARG;
    // R0, R1: the launches of the evaluation step
    Carver c(b->workspace, b->workspace_bytes);
    DCCN_TRY(rx_norm_r0(sh, L, b->x, b->x_norm, false, nullptr, rx_carve(c, L, RX_RECEIVE).norm, dccn_adam_hparams{}, 0, s));
    DCCN_TRY(cconv_fwd_impl(b->x_norm, P + L.o_conv_w, P + L.o_conv_b, b->fft_out, L.rows, sh->kin, sh->F, s));
    // R2 + decision
    if (via_tail_plan)
        return dense_decide_impl(b->fft_out, P + L.o_dense_w, P + L.o_dense_b, b->z, P + L.o_tail, b->packed, b->llr, b->prob,
                                 sh->batch, L.dK, L.dN, sh->nbits, s);
    DCCN_TRY(dense_fwd_impl(b->fft_out, P + L.o_dense_w, P + L.o_dense_b, b->z, sh->batch, L.dK, L.dN, s));
    return decide_impl(b->z, P + L.o_tail, b->packed, b->llr, b->prob, sh->batch, sh->D, sh->nbits, s);
}

// the stand-alone fused backward: the dense slabs' region, then the C-Conv partials' region
struct RxBackwardWs { void *dense, *conv; size_t n_dense, n_conv; };
static RxBackwardWs rx_backward_carve(Carver& c, int batch, int S, int kin, int F, int D) {
    const size_t nd = splitk_ws_bytes(S * 2 * F, 2 * D, batch), nc = rx_bwd_fused_ws_bytes(batch, S, kin, F);
    void* dense = c.take<char>(nd);
    return RxBackwardWs{dense, c.take<char>(nc), nd, nc};
}
}  // namespace dccn

using namespace dccn;

struct dccn_timer {
    hipEvent_t a, b;
};

extern "C" {

const char* dccn_strerror(int status) {
    switch (status) {
        case DCCN_OK: return "ok";
        case DCCN_ERR_INVALID_ARG: return "invalid argument";
        case DCCN_ERR_WORKSPACE: return "workspace missing or too small";
        case DCCN_ERR_LAUNCH: return "HIP launch/runtime error";
        case DCCN_ERR_NO_DEVICE: return "no HIP device visible";
        case DCCN_ERR_STATE: return "object used in the wrong state";
        case DCCN_ERR_UNSUPPORTED: return "a grouped call reached a launch that cannot carry several chains";
        default: return "unknown status";
    }
}

int dccn_version(void) { return 100; }
#ifndef DCCN_BUILD_ID
#define DCCN_BUILD_ID "unknown"
#endif
const char* dccn_build_id(void) { return DCCN_BUILD_ID; }
int dccn_last_hip_error(void) { return g_last_hip_error; }

int dccn_device_info(int* cu_count, int* wavefront, size_t* hbm_bytes, char* arch, int arch_len) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return DCCN_ERR_NO_DEVICE;
    int dev = 0;
    DCCN_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    DCCN_HIP(hipGetDeviceProperties(&prop, dev));
    if (cu_count) *cu_count = prop.multiProcessorCount;
    if (wavefront) *wavefront = prop.warpSize;
    if (hbm_bytes) *hbm_bytes = prop.totalGlobalMem;
    if (arch && arch_len > 0) {
        strncpy(arch, prop.gcnArchName, (size_t)arch_len - 1);
        arch[arch_len - 1] = 0;
    }
    return DCCN_OK;
}

size_t dccn_batch_moment_norm_workspace_size(int batch, int cols) {
    if (batch <= 0 || cols <= 0) return 0;
    return norm_ws_bytes(batch, cols);
}
int dccn_batch_moment_norm_fwd(const float* x, float* y, float* mean, float* var, int batch, int cols, float eps,
                               void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    dccn_adam_hparams hp;
    memset(&hp, 0, sizeof(hp));
    return norm_impl(x, y, mean, var, false, nullptr, batch, cols, eps, 8.0f, nullptr, hp, workspace, workspace_bytes,
                     (hipStream_t)stream);
}

size_t dccn_clip_power_workspace_size(long long n_pairs) {
    (void)n_pairs;
    return (size_t)4 * kCUs * sizeof(double);
}
int dccn_clip_power(const float* x, float* y, float* power_out, long long n_pairs, float peak, void* workspace,
                    size_t workspace_bytes, dccn_stream_t stream) {
    if (!x || !power_out || n_pairs <= 0) return DCCN_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < dccn_clip_power_workspace_size(n_pairs)) return DCCN_ERR_WORKSPACE;
    long long blocks = ceil_div_ll(n_pairs, 256);
    if (blocks > 4 * kCUs) blocks = 4 * kCUs;
    double* partial = static_cast<double*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(clip_power_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, y, n_pairs, peak, partial);
    DCCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, s, partial, (int)blocks, (double)n_pairs,
                       power_out);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

int dccn_cconv_gemm_fwd(const float* x, const float* w, const float* bias, float* out, int rows, int kin, int F,
                        dccn_stream_t stream) {
    return cconv_fwd_impl(x, w, bias, out, rows, kin, F, (hipStream_t)stream);
}
size_t dccn_cconv_gemm_bwd_w_workspace_size(int rows, int kin, int F) {
    if (rows <= 0 || kin <= 0 || F <= 0) return 0;
    return cconv_bw_ws_bytes(rows, kin, F);
}
int dccn_cconv_gemm_bwd_w(const float* x, const float* dout, float* dw, float* dbias, int rows, int kin, int F,
                          void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    return cconv_bwd_w_impl(x, dout, dw, dbias, rows, kin, F, workspace, workspace_bytes, (hipStream_t)stream);
}
int dccn_cconv_gemm_bwd_x(const float* dout, const float* w, float* dx, int rows, int kin, int F,
                          dccn_stream_t stream) {
    return cconv_bwd_x_impl(dout, w, dx, rows, kin, F, (hipStream_t)stream);
}

int dccn_dense_fwd(const float* x, const float* w, const float* bias, float* y, int M, int K, int N,
                   dccn_stream_t stream) {
    return dense_fwd_impl(x, w, bias, y, M, K, N, (hipStream_t)stream);
}
int dccn_dense_bwd_x(const float* dy, const float* w, float* dx, int M, int K, int N, dccn_stream_t stream) {
    return dense_bwd_x_impl(dy, w, dx, M, K, N, (hipStream_t)stream);
}
size_t dccn_dense_bwd_w_workspace_size(int M, int K, int N) {
    if (M <= 0 || K <= 0 || N <= 0) return 0;
    return splitk_ws_bytes(K, N, M);
}
int dccn_dense_bwd_w(const float* x, const float* dy, float* dw, float* dbias, int M, int K, int N, void* workspace,
                     size_t workspace_bytes, dccn_stream_t stream) {
    return dense_bwd_w_impl(x, dy, dw, dbias, M, K, N, workspace, workspace_bytes, (hipStream_t)stream);
}

int dccn_dense_bwd(const float* x, const float* dy, const float* w, float* dx, float* dw, float* dbias, int M, int K,
                   int N, void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DeferredSlabs ds;
    DCCN_TRY(dense_bwd_grouped_impl(x, dy, w, dx, dw, dbias, M, K, N, workspace, workspace_bytes, s, &ds));
    if (ds.dw_slabs) {
        const long long n = (long long)K * N;
        DCCN_TRY(launch_splitk_reduce(ds.dw_slabs, ds.splits, n, dw, n, s));
        if (dbias && ds.db_slabs) DCCN_TRY(launch_splitk_reduce(ds.db_slabs, ds.splits, (long long)N, dbias, (long long)N, s));
    }
    return DCCN_OK;
}

int dccn_dense_bwd_slabs(const float* x, const float* dy, const float* w, float* dx, float* dw, float* dbias, int M,
                         int K, int N, void* workspace, size_t workspace_bytes, int* splits, dccn_stream_t stream) {
    DeferredSlabs ds;
    DCCN_TRY(dense_bwd_grouped_impl(x, dy, w, dx, dw, dbias, M, K, N, workspace, workspace_bytes, (hipStream_t)stream,
                                    &ds));
    if (splits) *splits = ds.dw_slabs ? ds.splits : 1;
    return DCCN_OK;
}

// row[0..3] += conf, row[4] += ce_sum, row[5] += count  (one sweep-table row)
__global__ void metrics_table_add_kernel(const dccn_metrics* __restrict__ m, double* __restrict__ row) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        for (int k = 0; k < 4; ++k) row[k] += (double)m->conf[k];
        row[4] += m->ce_sum;
        row[5] += (double)m->count;
    }
}
int dccn_metrics_table_add(const dccn_metrics* metrics, double* row6, dccn_stream_t stream) {
    if (!metrics || !row6) return DCCN_ERR_INVALID_ARG;
    hipLaunchKernelGGL(metrics_table_add_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, metrics, row6);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}
// the training loop's per-step monitors (ofdmreceiver_np.py:222-229 fetches ce_mean, tx_power and the noise power of every step
// and averages them per epoch): acc3 += {ce_mean, tx_power, noise_power} in ONE single-thread launch instead of three framework
// launches -- same float32 additions in the same order
__global__ void step_monitor_add_kernel(const dccn_metrics* __restrict__ m, const float* __restrict__ tx_power,
                                        const float* __restrict__ noise_power, float* __restrict__ acc) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        acc[0] += m->ce_mean;
        if (tx_power) acc[1] += tx_power[0];
        if (noise_power) acc[2] += noise_power[0];
    }
}
int dccn_step_monitor_add(const dccn_metrics* metrics, const float* tx_power, const float* noise_power, float* acc3,
                          dccn_stream_t stream) {
    if (!metrics || !acc3) return DCCN_ERR_INVALID_ARG;
    DCCN_NO_CHAINS();
    hipLaunchKernelGGL(step_monitor_add_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, metrics, tx_power, noise_power, acc3);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}
// row = the record (a one-point table: no clearing launch in front of it)
__global__ void metrics_table_set_kernel(const dccn_metrics* __restrict__ m, double* __restrict__ row) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        for (int k = 0; k < 4; ++k) row[k] = (double)m->conf[k];
        row[4] = m->ce_sum;
        row[5] = (double)m->count;
    }
}
int dccn_metrics_table_set(const dccn_metrics* metrics, double* row6, dccn_stream_t stream) {
    if (!metrics || !row6) return DCCN_ERR_INVALID_ARG;
    hipLaunchKernelGGL(metrics_table_set_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, metrics, row6);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

static bool tune_key_live(int key) {
    return key >= 0 && key < TUNE_COUNT && key != 15 && key != 16 && key != 22 && key != 23 && key != 26;
}
int dccn_set_tuning(int key, int value) {
    if (!tune_key_live(key) || value < 0) return DCCN_ERR_INVALID_ARG;
    g_tune.set(key, value);
    if (key == TUNE_WHOLE_K) g_whole_k_global.store(value, std::memory_order_relaxed);
    return DCCN_OK;
}
int dccn_get_tuning(int key) { return (key < 0 || key >= TUNE_COUNT) ? DCCN_ERR_INVALID_ARG : g_tune.global(key); }
int dccn_tuning_count(void) { return TUNE_COUNT; }
int dccn_tuning_snapshot(int* table, int n) {
    if (!table || n < TUNE_COUNT) return DCCN_ERR_INVALID_ARG;
    for (int k = 0; k < TUNE_COUNT; ++k) table[k] = g_tune.global(k);
    return TUNE_COUNT;
}

size_t dccn_rx_backward_workspace_size(int batch, int S, int kin, int F, int D) {
    if (batch <= 0 || S <= 0 || kin <= 0 || F <= 0 || D <= 0) return 0;
    return carved_bytes([&](Carver& c) { rx_backward_carve(c, batch, S, kin, F, D); });
}
int dccn_rx_backward(const float* x_norm, const float* fft_out, const float* dz, const float* w_dense, float* dfft,
                     float* dw_dense, float* db_dense, float* dw_conv, float* db_conv, int batch, int S, int kin, int F,
                     int D, int reduce, void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    if (!x_norm || !fft_out || !dz || !w_dense || batch <= 0 || S <= 0 || kin <= 0 || F <= 0 || D <= 0)
        return DCCN_ERR_INVALID_ARG;
    if (reduce && (!dw_dense || !dw_conv)) return DCCN_ERR_INVALID_ARG;
    if (!rx_bwd_fused_ok(batch, S, kin, F, D, x_norm, fft_out, dz, w_dense)) return DCCN_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < dccn_rx_backward_workspace_size(batch, S, kin, F, D)) return DCCN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int dK = S * 2 * F, dN = 2 * D;
    Carver c(workspace, workspace_bytes);
    const RxBackwardWs w = rx_backward_carve(c, batch, S, kin, F, D);
    DeferredSlabs ds;
    FoldDefer fd;
    int tilew = 0;
    DCCN_TRY(rx_bwd_fused_impl(x_norm, fft_out, dz, w_dense, dfft, db_dense ? db_dense : dw_dense, batch, S, kin, F, D, w.dense,
                               w.n_dense, w.conv, w.n_conv, NormRideArgs{}, TailFinalizeArgs{}, dccn_adam_hparams{}, s, &ds, &fd, &tilew));
    if (!reduce) return DCCN_OK;
    const long long n = (long long)dK * dN;
    if (db_dense) DCCN_TRY(launch_splitk_reduce2(ds.dw_slabs, ds.splits, n, dw_dense, n, ds.db_slabs, (long long)dN, db_dense, (long long)dN, s));
    else DCCN_TRY(launch_splitk_reduce(ds.dw_slabs, ds.splits, n, dw_dense, n, s));
    const int fold_blocks = ceil_div(kin * F + F, tilew > 0 ? kFoldLanesTiled : kRedLanes);
    hipLaunchKernelGGL(cconv_fold_kernel, dim3(fold_blocks), dim3(256), 0, s, fd.slabs, fd.splits, fd.slab, fd.colsum, dw_conv,
                       db_conv, kin, F, tilew);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

size_t dccn_step_trace_bytes(int ring_steps) {
    if (ring_steps <= 0) return 0;
    return (size_t)ring_steps * kStampLaunches * kStampBlocks * kStampWords * sizeof(unsigned long long);
}
int dccn_step_trace_enable(unsigned long long* buf, size_t bytes, int ring_steps) {
    if (buf == nullptr) {
        g_step_trace.buf.store(nullptr);
        g_step_trace.ring.store(0);
        return DCCN_OK;
    }
    if (ring_steps <= 0 || bytes < dccn_step_trace_bytes(ring_steps)) return DCCN_ERR_WORKSPACE;
    g_step_trace.ring.store(ring_steps);
    g_step_trace.step.store(0);
    g_step_trace.buf.store(buf);
    return DCCN_OK;
}
long long dccn_step_trace_steps(void) { return g_step_trace.step.load(); }
void dccn_step_trace_geometry(int* launches, int* blocks, int* words) {
    if (launches) *launches = kStampLaunches;
    if (blocks) *blocks = kStampBlocks;
    if (words) *words = kStampWords;
}

#ifdef DCCN_TRACE
/* trace build only (tools/blocktrace.py): where the instrumented kernels leave their per-block time stamps */
int dccn_debug_set_trace(unsigned long long* buf) {
    DCCN_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_trace), &buf, sizeof(buf)));
    return DCCN_OK;
}
#endif

int dccn_dense_tail_supported(int M, int K, int N, int nbits) { return dense_tail_shape_ok(M, K, N, nbits) ? 1 : 0; }
// (the description dense_tail_impl / dense_decide_impl build, on null -- 16-byte aligned -- operands: nothing is read)
int dccn_dense_tail_grid(int M, int K, int N, int nbits, int* grid, int* tile_rows, int* ragged_rows, int* blocks) {
    const TuneScope tune;
    if (!dense_tail_ok(nullptr, nullptr, M, K, N, nbits)) return DCCN_ERR_INVALID_ARG;
    const DenseRoute r = dense_tail_route(dense_fwd_params(nullptr, nullptr, nullptr, nullptr, M, K, N), nbits);
    if (grid) *grid = r.grid;
    if (tile_rows) *tile_rows = r.grid == DG_FEWROW ? 16 : (r.grid == DG_RAGGED || r.large) ? kDense80.rows() : kDense48.rows();
    if (ragged_rows) *ragged_rows = r.grid == DG_RAGGED ? r.rag : 0;
    if (blocks) *blocks = r.blocks;
    return DCCN_OK;
}
// (the descriptions the *_impl functions build, on null -- 16-byte aligned -- inputs and a 16-byte aligned output address that
// nothing dereferences: the few-row and k-major tiles ask for an output and its alignment)
int dccn_gemm_route_query(int op, int d0, int d1, int d2, int d3, int d4, dccn_gemm_route* route) {
    const TuneScope tune;
    float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(256));
    if (!route || d0 <= 0 || d1 <= 0 || d2 <= 0) return DCCN_ERR_INVALID_ARG;
    Route r;
    switch (op) {
        case DCCN_ROUTE_DENSE_FWD:
            DCCN_TRY(dense_fwd_route(dense_fwd_params(nullptr, nullptr, nullptr, out, d0, d1, d2), STORE_PLAIN, &r));
            break;
        case DCCN_ROUTE_DENSE_BWD_X:
            DCCN_TRY(dense_bwd_x_route(dense_bwd_x_params(nullptr, nullptr, out, d0, d1, d2), &r));
            break;
        case DCCN_ROUTE_DENSE_BWD_W: {
            const SplitPlan sp = dense_dw_plan(d0, d1, d2);
            GemmParams p = dense_bwd_w_params(nullptr, nullptr, d0, d1, d2);
            p.klen = sp.klen; p.C = out;
            r = dense_bwd_w_route(p, sp);
            break;
        }
        case DCCN_ROUTE_DENSE_BWD: {
            GemmParams pw = dense_bwd_w_params(nullptr, nullptr, d0, d1, d2);
            pw.C = out;
            DCCN_TRY(dense_bwd_route(dense_bwd_x_params(nullptr, nullptr, out, d0, d1, d2), pw, d0, d1, d2, 1, false, &r));
            break;
        }
        case DCCN_ROUTE_CCONV_FWD:
            r = cconv_fwd_route(cconv_fwd_params(nullptr, nullptr, nullptr, out, d0, d1, d2), d1);
            break;
        case DCCN_ROUTE_CCONV_BWD_W: {
            GemmParams p = cconv_bwd_w_params(nullptr, nullptr, d0, d1, d2);
            p.C = out;
            DCCN_TRY(cconv_bwd_w_route(p, d0, d1, d2, true, &r));
            break;
        }
        case DCCN_ROUTE_RX_BACKWARD: {
            if (d3 <= 0 || d4 <= 0 || !rx_bwd_fused_ok(d0, d1, d2, d3, d4, nullptr, nullptr, nullptr, nullptr)) return DCCN_ERR_INVALID_ARG;
            const int dK = d1 * 2 * d3, dN = 2 * d4;
            GemmParams pw = dense_bwd_w_params(nullptr, nullptr, d0, dK, dN);
            if (!vec_both(pw)) return DCCN_ERR_INVALID_ARG;
            pw.C = out;
            DCCN_TRY(rx_bwd_route(pw, d0, dK, dN, &r));
            break;
        }
        default: return DCCN_ERR_INVALID_ARG;
    }
    *route = r;
    return DCCN_OK;
}
int dccn_rx_dense_tail_fused(const dccn_rx_shape* sh, int train) {
    return shape_ok(sh) && rx_dense_tail_fused_ok(sh, train != 0, nullptr, nullptr) ? 1 : 0;
}
// (pointer alignment is checked again when a step is planned; the queries assume 16-byte aligned buffers)
int dccn_rx_bwd_fused_supported(const dccn_rx_shape* sh) {
    return shape_ok(sh) && rx_bwd_fused_ok(sh, nullptr, nullptr, nullptr, nullptr) ? 1 : 0;
}
int dccn_rx_norm_rides_backward(const dccn_rx_shape* sh) {
    return dccn_rx_bwd_fused_supported(sh) && rx_norm_rides_bwd_ok(sh, true, nullptr, nullptr) ? 1 : 0;
}
int dccn_rx_gen_next_supported(const dccn_rx_shape* sh) {
    return shape_ok(sh) && !dccn_rx_norm_rides_backward(sh) && rx_gen_next_ok(sh, nullptr, nullptr) ? 1 : 0;
}

size_t dccn_dense_tail_workspace_size(int M, int N, int nbits) {
    if (M <= 0 || N <= 0 || nbits < 1 || nbits > 4) return 0;
    return dense_tail_ws_bytes(M, N, nbits);
}
int dccn_dense_tail_fwd(const float* x, const float* w, const float* bias, float* z, const int32_t* bits,
                        const float* tailp, float* prob, dccn_metrics* metrics, int M, int K, int N, int nbits,
                        void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    return dense_tail_impl(false, x, w, bias, z, bits, tailp, prob, metrics, nullptr, nullptr, M, K, N, nbits, nullptr,
                           nullptr, workspace, workspace_bytes, (hipStream_t)stream);
}
int dccn_dense_tail_fwd_bwd(const float* x, const float* w, const float* bias, float* z, const int32_t* bits,
                            const float* tailp, float* prob, dccn_metrics* metrics, float* dz, float* dtailp, int M,
                            int K, int N, int nbits, void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    return dense_tail_impl(true, x, w, bias, z, bits, tailp, prob, metrics, dz, dtailp, M, K, N, nbits, nullptr, nullptr,
                           workspace, workspace_bytes, (hipStream_t)stream);
}

int dccn_demod_decide(const float* z, const float* tailp, unsigned char* packed, float* llr, float* prob, int frames, int D,
                      int nbits, dccn_stream_t stream) {
    return decide_impl(z, tailp, packed, llr, prob, frames, D, nbits, (hipStream_t)stream);
}
int dccn_dense_decide_supported(int M, int K, int N, int nbits) {
    const TuneScope tune;
    return (nbits >= 1 && nbits <= 4 && N > 0 && (N & 1) == 0 && dense_tail_shape_ok(M, K, N, nbits)) ? 1 : 0;
}
int dccn_dense_decide_fwd(const float* x, const float* w, const float* bias, float* z, const float* tailp,
                          unsigned char* packed, float* llr, float* prob, int M, int K, int N, int nbits,
                          dccn_stream_t stream) {
    const TuneScope tune;
    return dense_decide_impl(x, w, bias, z, tailp, packed, llr, prob, M, K, N, nbits, (hipStream_t)stream);
}
size_t dccn_rx_receive_workspace_size(const dccn_rx_shape* shape) {
    if (!shape_ok(shape)) return 0;
    return rx_ws_bytes(shape, RX_RECEIVE);
}
int dccn_rx_receive_fused(const dccn_rx_shape* shape) {
    if (!shape_ok(shape)) return 0;
    const TuneScope tune;
    return rx_receive_fused(shape, rx_dense_tail_fused_ok(shape, false, nullptr, nullptr)) ? 1 : 0;
}
int dccn_rx_receive_step(const dccn_rx_shape* shape, const dccn_rx_receive_buffers* buf, dccn_stream_t stream) {
    return rx_receive_impl(shape, buf, (hipStream_t)stream);
}

int dccn_tail_param_count(int nbits) {
    if (nbits < 1 || nbits > 4) return DCCN_ERR_INVALID_ARG;
    return tail_param_count(nbits);
}
size_t dccn_demod_tail_workspace_size(long long cells, int nbits) {
    if (cells <= 0 || nbits < 1 || nbits > 4) return 0;
    return tail_ws_bytes(cells, nbits);
}
int dccn_demod_tail_loss_fwd(const float* z, const int32_t* bits, const float* tailp, float* prob,
                             dccn_metrics* metrics, long long cells, int nbits, void* workspace,
                             size_t workspace_bytes, dccn_stream_t stream) {
    return tail_impl(false, z, bits, tailp, prob, metrics, nullptr, nullptr, cells, nbits, nullptr, nullptr, workspace,
                     workspace_bytes, (hipStream_t)stream);
}
int dccn_demod_tail_loss_fwd_bwd(const float* z, const int32_t* bits, const float* tailp, float* prob,
                                 dccn_metrics* metrics, float* dz, float* dtailp, long long cells, int nbits,
                                 void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    return tail_impl(true, z, bits, tailp, prob, metrics, dz, dtailp, cells, nbits, nullptr, nullptr, workspace,
                     workspace_bytes, (hipStream_t)stream);
}

int dccn_adam_tf_step(float* param, const float* grad, float* m, float* v, const float* reg_coef,
                      const float* reg_gate, dccn_adam_state* state, dccn_adam_hparams hp, long long n,
                      dccn_stream_t stream) {
    return adam_impl(param, grad, m, v, reg_coef, reg_gate, state, hp, n, (hipStream_t)stream);
}

int dccn_rx_param_offsets(const dccn_rx_shape* shape, long long offsets[6]) {
    if (!shape_ok(shape) || !offsets) return DCCN_ERR_INVALID_ARG;
    const RxLayout L = rx_layout(shape);
    offsets[0] = L.o_conv_w; offsets[1] = L.o_conv_b; offsets[2] = L.o_dense_w;
    offsets[3] = L.o_dense_b; offsets[4] = L.o_tail; offsets[5] = L.total;
    return DCCN_OK;
}
size_t dccn_rx_workspace_size(const dccn_rx_shape* shape, int train) {
    // the library's second stream and the calling thread's event pair are created here, i.e. before any step and outside
    // any stream capture (every caller sizes its workspace first); rx_step_impl only looks them up
    if (train && shape_ok(shape) && g_tune[TUNE_ADAM_OVERLAP]) { OverlapStreams o; (void)overlap_streams(&o); }
    if (!shape_ok(shape)) return 0;
    return rx_ws_bytes(shape, train ? RX_TRAIN : RX_EVAL);
}
int dccn_rx_eval_step(const dccn_rx_shape* shape, const dccn_rx_buffers* buf, dccn_stream_t stream) {
    return rx_step_impl(shape, buf, false, dccn_adam_hparams{}, (hipStream_t)stream, nullptr);
}
int dccn_rx_train_step(const dccn_rx_shape* shape, const dccn_rx_buffers* buf, dccn_adam_hparams hp,
                       dccn_stream_t stream) {
    return rx_step_impl(shape, buf, true, hp, (hipStream_t)stream, nullptr);
}
// R0 (+R8 partial sums) of buf->x into buf->x_norm exactly as a step would run it: primes the pipelined mode
// (dccn_rx_buffers.x_prenormalised) before the first call
int dccn_rx_normalise(const dccn_rx_shape* shape, const dccn_rx_buffers* buf, dccn_stream_t stream) {
    if (!shape_ok(shape) || !buf || !buf->x || !buf->x_norm) return DCCN_ERR_INVALID_ARG;
    if (!buf->workspace || buf->workspace_bytes < rx_ws_bytes(shape, RX_TRAIN)) return DCCN_ERR_WORKSPACE;
    PowerPartials pp;
    const RxLayout L = rx_layout(shape);
    Carver c(buf->workspace, buf->workspace_bytes);
    return rx_norm_r0(shape, L, buf->x, buf->x_norm, buf->tx_power != nullptr, &pp, rx_carve(c, L, RX_TRAIN).norm, dccn_adam_hparams{},
                      buf->norm_slot ? 1 : 0, (hipStream_t)stream);
}

// mode: bit0 = train, bit1 = fork the dense weight-gradient branch onto a second stream
int dccn_rx_graph_create(const dccn_rx_shape* shape, const dccn_rx_buffers* buf, int mode, dccn_adam_hparams hp,
                         dccn_stream_t stream, dccn_rx_graph** out) {
    if (!out || !shape_ok(shape) || !buf) return DCCN_ERR_INVALID_ARG;
    const bool train = mode & 1, fork = (mode & 2) && train;
    (void)stream;
    return graph_capture(fork, out, [&](const dccn_rx_graph& g) {
        const OverlapStreams branch{g.side, g.ev_fork, g.ev_join};
        return rx_step_impl(shape, buf, train, hp, g.cap, fork ? &branch : nullptr);
    });
}
// ---- HIP-event timers on the caller's stream ------------------------------------------------------------------
int dccn_timer_create(dccn_timer** out) {
    if (!out) return DCCN_ERR_INVALID_ARG;
    dccn_timer* t = new dccn_timer();
    if (hipEventCreate(&t->a) != hipSuccess || hipEventCreate(&t->b) != hipSuccess) {
        delete t;
        return DCCN_ERR_LAUNCH;
    }
    *out = t;
    return DCCN_OK;
}
int dccn_timer_start(dccn_timer* t, dccn_stream_t stream) {
    if (!t) return DCCN_ERR_STATE;
    DCCN_HIP(hipEventRecord(t->a, (hipStream_t)stream));
    return DCCN_OK;
}
int dccn_timer_stop(dccn_timer* t, dccn_stream_t stream) {
    if (!t) return DCCN_ERR_STATE;
    DCCN_HIP(hipEventRecord(t->b, (hipStream_t)stream));
    return DCCN_OK;
}
int dccn_timer_elapsed_ms(dccn_timer* t, float* ms) {
    if (!t || !ms) return DCCN_ERR_STATE;
    DCCN_HIP(hipEventSynchronize(t->b));
    DCCN_HIP(hipEventElapsedTime(ms, t->a, t->b));
    return DCCN_OK;
}
int dccn_timer_destroy(dccn_timer* t) {
    if (!t) return DCCN_OK;
    (void)hipEventDestroy(t->a);
    (void)hipEventDestroy(t->b);
    delete t;
    return DCCN_OK;
}

}  // extern "C"
