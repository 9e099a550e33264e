// Fused equaliser transfer-learning step: dev/py/ofdmreceiver_np_mp.py:283-330 as one
// pre-planned launch sequence (capturable into a hipGraph) over flat arenas --
//   R0 normalise -> equalizer_ofdm (model.py:349-478) -> frozen basic receiver -> loss/BER
//   -> backward to the Equalizer/* variables only -> TF Adam on the equaliser arena.
// Included inside namespace dccn of dccn_abi_eq.hip, behind abi_impl.h (the operators' *_impl launch planning it is built from).
// eq_step_plan checks every argument and makes every decision (EqStepPlan) and launches nothing; eq_issue_forward / _rx /
// _backward / _update only read the plan.  The dccn_eq_* queries ask the plan's own predicates.
// FLAGS.cp=False (model.py:364-366, 1236-1240): the equaliser's first dense layer and the receiver's C-Conv read
// the K-sample window behind the cyclic prefix of [.., n_sc, 2] rows -- a column window of the same buffers.

static bool eq_shape_ok(const dccn_eq_shape* sh) {
    return sh && sh->batch > 0 && sh->S > 0 && sh->K > 0 && sh->CP >= 0 && sh->F > 0 && sh->D > 0 && sh->nbits >= 1 &&
           sh->nbits <= 4 && sh->pilot_size > 0 && (sh->cp == 0 || sh->cp == 1);
}

struct EqDims {
    int B, S, K, nsc, R, SK2, Pp, F, D, cp, win;     // win: float offset of the post-CP window inside a row
    long long o[21];        // parameter offsets, TF creation order (dense, conv3d, dense_1..4, conv3d_1..3, dense_5)
    long long sz[20];       // element counts (o[i+1] - o[i] may include up to three floats of alignment padding)
};
static EqDims eq_dims(const dccn_eq_shape* sh) {
    EqDims d;
    d.B = sh->batch; d.S = sh->S; d.K = sh->K; d.nsc = sh->K + sh->CP; d.R = d.B * d.S;
    d.SK2 = d.S * d.K * 2; d.Pp = 2 * sh->pilot_size; d.F = sh->F; d.D = sh->D;
    d.cp = sh->cp; d.win = sh->cp ? 0 : 2 * sh->CP;
    const long long K2 = 2LL * d.K, N2 = 2LL * d.nsc, SK2 = d.SK2;
    const long long sizes[20] = {(sh->cp ? N2 : K2) * K2, K2,   // dense (input: whole row, or the window)
                                 (long long)d.K * K2, K2,     // conv3d     (1,K) -> K filters
                                 SK2 * d.Pp, d.Pp,            // dense_1    pilot extraction
                                 d.Pp * SK2, SK2,             // dense_2
                                 SK2 * SK2, SK2,              // dense_3
                                 SK2 * SK2, SK2,              // dense_4    (tanh)
                                 SK2, 2,                      // conv3d_1   (S,K) -> 1 filter
                                 (long long)d.K * K2, K2,     // conv3d_2   (corr)
                                 (long long)d.K * K2, K2,     // conv3d_3   (equalized)
                                 4LL * d.K * N2, N2};         // dense_5
    // every tensor starts on a 16-byte boundary (padding floats stay zero: zero gradient, zero Adam slots): the
    // two-float bias of conv3d_1 used to shift conv3d_2 / conv3d_3 / dense_5 off it, and their five GEMMs onto the
    // element-wise masked loaders -- 45 us of the 374 us step at 73 frames (profiles/r03_eq73_kernel_stats.txt)
    d.o[0] = 0;
    for (int i = 0; i < 20; ++i) { d.o[i + 1] = (d.o[i] + sizes[i] + 3) / 4 * 4; d.sz[i] = sizes[i]; }
    return d;
}

// weight-gradient workspaces, one per trainable layer (their slabs stay live until the optimizer launch reduces them)
enum EqLayer : int { EQL_DENSE = 0, EQL_CONV, EQL_DENSE1, EQL_DENSE2, EQL_DENSE3, EQL_DENSE4, EQL_SMOOTH, EQL_PAIR, EQL_DENSE5,
                     EQL_COUNT };
struct EqWs {
    void *ws_norm, *ws_tail;
    void* ws_l[EQL_COUNT];
    size_t n_norm, n_tail, n_l[EQL_COUNT];
    float *x_norm, *ln, *t1, *y, *d1, *d2, *d3, *d4, *T, *be, *eq, *corr, *eqc, *corc, *cat, *fft, *z;
    // training only
    float *dz, *dfft, *dout, *dcat, *deqc, *dcorc, *deq, *dcorr, *dy, *dh, *dT, *dbe, *dd4, *dd3, *dd2, *dd1,
        *dflat, *dt1, *dtail;
    float* bn_part;          // per-block weight-gradient partials of the fused bottleneck backward (eq_bottleneck.h)
};
static void eq_layer_ws(const EqDims& d, size_t (&n)[EQL_COUNT]) {
    n[EQL_DENSE] = splitk_ws_bytes(d.cp ? 2 * d.nsc : 2 * d.K, 2 * d.K, d.R);
    n[EQL_CONV] = cconv_bwd_grouped_ws_bytes(d.R, d.K, d.K, 1);
    n[EQL_DENSE1] = splitk_ws_bytes(d.SK2, d.Pp, d.B);
    n[EQL_DENSE2] = splitk_ws_bytes(d.Pp, d.SK2, d.B);
    n[EQL_DENSE3] = n[EQL_DENSE4] = n[EQL_SMOOTH] = splitk_ws_bytes(d.SK2, d.SK2, d.B);
    n[EQL_PAIR] = cconv_bwd_grouped_ws_bytes(d.R, d.K, d.K, 2);           // corr and eq C-Convs
    n[EQL_DENSE5] = splitk_ws_bytes(4 * d.K, 2 * d.nsc, d.R);
}
// The float tensors of the workspace, in carve order (the order IS the layout): name (dccn_eq_workspace_tensor; null: not offered
// by name), member, element count for a shape, training only.  eq_carve and the lookup by name both walk this table.
struct EqWsTensor { const char* name; float* EqWs::*member; size_t (*count)(const EqDims&); bool train; };
static size_t eqn_rows_nsc(const EqDims& d) { return (size_t)d.R * 2 * d.nsc; }         // [B, S, n_sc, 2]
static size_t eqn_rows_k(const EqDims& d) { return (size_t)d.R * 2 * d.K; }             // [B*S, K, 2]
static size_t eqn_rows_2k(const EqDims& d) { return (size_t)d.R * 4 * d.K; }            // [B*S, K, 4]
static size_t eqn_rows_f(const EqDims& d) { return (size_t)d.R * 2 * d.F; }
static size_t eqn_frames(const EqDims& d) { return (size_t)d.B * d.SK2; }               // [B, S*K*2]
static size_t eqn_pilots(const EqDims& d) { return (size_t)d.B * d.Pp; }
static size_t eqn_cells(const EqDims& d) { return (size_t)d.B * 2 * d.D; }
static size_t eqn_smooth(const EqDims& d) { return (size_t)d.SK2 * d.SK2; }
static size_t eqn_smooth_b(const EqDims& d) { return (size_t)d.SK2; }
static size_t eqn_tail(const EqDims&) { return (size_t)tail_param_count(4); }
static size_t eqn_bn_part(const EqDims& d) { return (d.Pp == 16 || d.Pp == 32) ? eq_bottleneck_part_floats(d.B, d.SK2, d.Pp) : 0; }
static const EqWsTensor kEqWsTensors[] = {
    {"x_norm", &EqWs::x_norm, eqn_rows_nsc, false}, {"ln", &EqWs::ln, eqn_rows_nsc, false}, {"t1", &EqWs::t1, eqn_rows_k, false},
    {"y", &EqWs::y, eqn_rows_k, false}, {"d1", &EqWs::d1, eqn_pilots, false}, {"d2", &EqWs::d2, eqn_frames, false},
    {"d3", &EqWs::d3, eqn_frames, false}, {"d4", &EqWs::d4, eqn_frames, false}, {"T", &EqWs::T, eqn_smooth, false},
    {"be", &EqWs::be, eqn_smooth_b, false}, {"eq", &EqWs::eq, eqn_frames, false}, {"corr", &EqWs::corr, eqn_frames, false},
    {"eqc", &EqWs::eqc, eqn_rows_k, false}, {"corc", &EqWs::corc, eqn_rows_k, false}, {"cat", &EqWs::cat, eqn_rows_2k, false},
    {"fft", &EqWs::fft, eqn_rows_f, false}, {"z", &EqWs::z, eqn_cells, false},
    {"dz", &EqWs::dz, eqn_cells, true}, {"dfft", &EqWs::dfft, eqn_rows_f, true}, {"dout", &EqWs::dout, eqn_rows_nsc, true},
    {"dcat", &EqWs::dcat, eqn_rows_2k, true}, {"deqc", &EqWs::deqc, eqn_rows_k, true}, {"dcorc", &EqWs::dcorc, eqn_rows_k, true},
    {"deq", &EqWs::deq, eqn_frames, true}, {"dcorr", &EqWs::dcorr, eqn_frames, true}, {"dy", &EqWs::dy, eqn_frames, true},
    {"dh", &EqWs::dh, eqn_frames, true}, {"dT", &EqWs::dT, eqn_smooth, true}, {"dbe", &EqWs::dbe, eqn_smooth_b, true},
    {"dd4", &EqWs::dd4, eqn_frames, true}, {"dd3", &EqWs::dd3, eqn_frames, true}, {"dd2", &EqWs::dd2, eqn_frames, true},
    {"dd1", &EqWs::dd1, eqn_pilots, true}, {"dflat", &EqWs::dflat, eqn_frames, true}, {"dt1", &EqWs::dt1, eqn_rows_k, true},
    {nullptr, &EqWs::dtail, eqn_tail, true}, {nullptr, &EqWs::bn_part, eqn_bn_part, true},
};
// each(tensor, byte offset, count): called for every float tensor the workspace holds
template <typename Each>
static void eq_carve(Carver& c, const EqDims& d, bool train, EqWs& w, Each&& each) {
    w.n_norm = norm_ws_bytes(d.B, d.S * d.nsc * 2);
    // the layout does not depend on the modulation (the tail's slabs and gradient are sized for 16-QAM): chains of different
    // modulations carried by one launch sequence (dccn_eq_train_step_grouped) see the same offsets
    w.n_tail = 0;
    for (int nb = 1; nb <= 4; ++nb) {
        const size_t t = tail_ws_bytes((long long)d.B * d.D, nb), f = dense_tail_ws_bytes(d.B, 2 * d.D, nb);
        if (t > w.n_tail) w.n_tail = t;
        if (f > w.n_tail) w.n_tail = f;
    }
    w.ws_norm = c.take<char>(w.n_norm);
    w.ws_tail = c.take<char>(w.n_tail);
    eq_layer_ws(d, w.n_l);
    for (int l = 0; l < EQL_COUNT; ++l) w.ws_l[l] = train ? c.take<char>(w.n_l[l]) : nullptr;
    for (const EqWsTensor& t : kEqWsTensors) {
        if (t.train && !train) continue;
        const size_t n = t.count(d);
        w.*t.member = c.take<float>(n);
        each(t, c.off - n * sizeof(float), n);
    }
}
static void eq_carve(Carver& c, const EqDims& d, bool train, EqWs& w) {
    eq_carve(c, d, train, w, [](const EqWsTensor&, size_t, size_t) {});
}
static size_t eq_ws_bytes(const dccn_eq_shape* sh, int train) {
    return carved_bytes([&](Carver& c) { EqWs w; eq_carve(c, eq_dims(sh), train != 0, w); });
}

// dense backward with reduced outputs: dx (nullable: weight gradient only), dw, dbias
// actx / aux / act_done: optional element-wise stage on the dX store (dense_bwd_grouped_impl)
// keep: leave split-K slabs un-reduced and report them (the optimizer launch sums them, eq_opt.h)
// split_dst / split_gc / split_done: dx is the gradient of a concat of two IQ-pair streams; when the launch plan has the
// stage, the streams' own buffers are written instead of dx (dense_bwd_grouped_impl)
static int dense_bwd_full_impl(const float* x, const float* dy, const float* w, float* dx, float* dw, float* dbias,
                               int M, int K, int N, void* ws, size_t ws_bytes, hipStream_t s, int actx = 1,
                               const float* aux = nullptr, bool* act_done = nullptr, DeferredSlabs* keep = nullptr,
                               float* split_dst = nullptr, long long split_gc = 0, bool* split_done = nullptr) {
    if (act_done) *act_done = false;
    if (split_done) *split_done = false;
    DeferredSlabs ds;
    if (!dx) {
        DCCN_TRY(dense_bwd_w_impl(x, dy, dw, dbias, M, K, N, ws, ws_bytes, s, keep));
        return DCCN_OK;
    }
    DCCN_TRY(dense_bwd_grouped_impl(x, dy, w, dx, dw, dbias, M, K, N, ws, ws_bytes, s, &ds, actx, aux, act_done,
                                    split_dst, split_gc, split_done));
    if (keep) {
        *keep = ds;
        return DCCN_OK;
    }
    if (ds.dw_slabs) {
        const long long n = (long long)K * N;
        if (dbias && ds.db_slabs)
            DCCN_TRY(launch_splitk_reduce2(ds.dw_slabs, ds.splits, n, dw, n, ds.db_slabs, (long long)N, dbias, (long long)N, s));
        else
            DCCN_TRY(launch_splitk_reduce(ds.dw_slabs, ds.splits, n, dw, n, s));
    }
    return DCCN_OK;
}

// optimizer jobs of a dense layer (kernel variable i, bias variable i + 1)
// (uni: the caller's reg_coef is one value over each dense kernel / bias -- dccn_eq_buffers.reg_uniform)
// kernel_done: the kernel variable was updated by a rider of an earlier launch (EqRideArgs)
static void eq_opt_dense(EqOptBuilder& ob, const EqDims& d, int i, const DeferredSlabs& ds, long long N, bool uni,
                         bool kernel_done = false) {
    if (kernel_done) {}
    else if (ds.dw_slabs) ob.slabs(d.o[i], d.sz[i], ds.dw_slabs, ds.splits, d.sz[i], uni);
    else ob.plain(d.o[i], d.sz[i], uni);
    if (ds.dw_slabs && ds.db_slabs) ob.slabs(d.o[i + 1], d.sz[i + 1], ds.db_slabs, ds.splits, N, uni);
    else ob.plain(d.o[i + 1], d.sz[i + 1], uni);
}

// ---- what a step launches for a shape: each condition is spelled ONCE.  The dccn_eq_* queries ask with null pointers
// ("given 16-byte aligned buffers"), the step's plan asks with the caller's buffers. ----
// the frozen receiver as the equaliser feeds it (cp = 0: the K-sample window behind the cyclic prefix)
static dccn_rx_shape eq_rx_shape(const EqDims& d, int nbits) {
    return dccn_rx_shape{d.B, d.S, d.cp ? d.nsc : d.K, d.F, d.D, nbits};
}
// `input:0` by the single-pass kernel (one launch, and one that carries a chain index) ...
static bool eq_norm_single_ok(const EqDims& d, const float* x, const float* x_norm) {
    return g_tune[TUNE_EQ_REPLAN] != 0 && kNormFusedCG == 2 && norm_fused_ok(x, x_norm, d.B, d.S * 2 * d.nsc);
}
// ... the optimizer launch of a training step can then run it for the NEXT batch
static bool eq_norm_rides_ok(const EqDims& d, bool train, const float* x, const float* x_norm) {
    return train && eq_norm_single_ok(d, x, x_norm);
}
// both layers of the pilot bottleneck in one launch per direction (eq_bottleneck.h); W1 / W2: the dense_1 / dense_2 kernels
static bool eq_bn_ok(const EqDims& d, const float* y, const float* W1, const float* W2, const float* d1) {
    return g_tune[TUNE_EQ_REPLAN] == 1 && eq_bottleneck_ok(d.B, d.SK2, d.Pp, y, W1, W2) && aligned16(d1);
}
// few rows (73 frames): the fused dense + tail launch is 20 tiles of 48x64 behind a 14-tile k-loop (23 us); the
// one-latency 16x16 tiles of fewrow.h (200 blocks) followed by the stand-alone tail launch take about half of that
static bool eq_few_rx_ok(const EqDims& d, const RxLayout& L, const float* fft, const float* rx_params, const float* z) {
    return g_tune[TUNE_FEWROW] && g_tune[TUNE_SKINNY] > 0 && d.B <= 96 && (L.dK % 16) == 0 && L.dK >= 128 && L.dK <= 1152 &&
           (L.dN % 16) == 0 && aligned16(fft) && aligned16(z) &&
           ((reinterpret_cast<uintptr_t>(rx_params) + 4 * (uintptr_t)L.o_dense_w) & 15u) == 0;      // (the dense kernel)
}
// ... and with the receiver's C-Conv and dense layer folded into one matrix (dccn_eq_rx_fold: the receiver is frozen)
// both run as ONE such GEMM over the flattened frame, K = S * 2 n_sc
static bool eq_rx_folded_ok(const EqDims& d, bool few_rx, const float* Mf, const float* out_eq) {
    const int fK = d.S * 2 * d.nsc;
    return few_rx && g_tune[TUNE_FEWROW] >= 1 && aligned16(Mf) && aligned16(out_eq) && (fK % 16) == 0 && fK <= 1152;
}
// a chain group (common.h ChainCtx) runs on the launches that carry a chain index: the single-pass normalisation, the
// bottleneck as one launch per direction, the few-row plan with the receiver folded into one matrix
static bool eq_group_ok(bool rides, bool bn, bool folded) { return rides && bn && folded; }
// ... and a forward-only group (dccn_eq_receive_step_grouped) on the same forward launches: no optimizer launch, so the
// normalisation is asked for as the step's own single-pass launch
static bool eq_receive_group_ok(bool norm_single, bool bn, bool folded) { return norm_single && bn && folded; }
// per-block weight-gradient partials of the fused bottleneck backward, summed by a later launch
struct EqBnParts { float *w2, *b2, *w1, *b1; int tiles; };      // [tiles][P][SK2], [tiles][SK2], [tiles][SK2][P], [tiles][P]
static EqBnParts eq_bn_parts(float* base, int B, int SK2, int P) {
    const size_t t = ceil_div(B, 16);
    float *w2 = base, *b2 = w2 + t * P * SK2, *w1 = b2 + t * SK2, *b1 = w1 + t * SK2 * P;
    return EqBnParts{w2, b2, w1, b1, (int)t};
}

// the two launches of the pilot bottleneck: kernel by P, q, the grid and the argument order.  The backward launch can carry riders
// (EqRideArgs jobs behind its own blocks, the next batch's generator in front of them: eq_issue_backward); the stage operators
// pass eq_bn_no_riders()
static int eq_bottleneck_fwd_launch(const float* y, const float* W1, const float* b1, const float* W2, const float* b2, float* d1,
                                    float* d2, int B, int SK2, int P, hipStream_t s) {
    auto kern = P == 32 ? eq_bottleneck_fwd_kernel<2> : eq_bottleneck_fwd_kernel<1>;
    const int q = eq_bottleneck_q(B, SK2);
    DCCN_LAUNCH_CHAINS_Z(kern, dim3(ceil_div(SK2 / 16, q), ceil_div(B, 16)), dim3(256), 0, s, y, W1, b1, W2, b2, d1, d2, B, SK2, q);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}
struct EqBnRiders {
    EqRideArgs ride;
    dccn_adam_hparams hp;
    int gen_blocks;                 // workgroups of the generator (they fill the first grid rows), 0: none
    size_t gen_smem;
    GenStaticArgs ga;
    GenChainScalars gc;
};
static EqBnRiders eq_bn_no_riders() {
    EqBnRiders r;
    memset(&r, 0, sizeof(r));
    return r;
}
static int eq_bottleneck_bwd_launch(const float* dd2, const float* d1, const float* y, const float* W1, const float* W2,
                                    const float* dy_in, float* dy_out, const EqBnParts& pt, int B, int SK2, int P, const EqBnRiders& r,
                                    hipStream_t s) {
    auto kern = P == 32 ? eq_bottleneck_bwd_kernel<2> : eq_bottleneck_bwd_kernel<1>;
    const int q = eq_bottleneck_q(B, SK2);
    const int nx = ceil_div(SK2 / 16, q), gen_rows = ceil_div(r.gen_blocks, nx);
    DCCN_LAUNCH_CHAINS_Z(kern, dim3(nx, gen_rows + pt.tiles + ceil_div(r.ride.blocks, nx)), dim3(256), r.gen_smem, s, dd2, d1, y, W1, W2,
                         dy_in, dy_out, pt.w2, pt.b2, pt.w1, pt.b1, B, SK2, q, pt.tiles, r.ride, r.hp, gen_rows, r.gen_blocks, r.ga, r.gc);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

// the monitors' launch (equalizer.h eq_monitor_kernel): its grid, its workspace -- the blocks' arrival counter, one partial sum per
// block -- and its argument block from the caller's descriptor, for the stand-alone launch and for the step's optimizer launch
static int eq_monitor_blocks(int B, int K) {
    long long n = ceil_div_ll((long long)B * K * 2, 256);
    if (n > 256) n = 256;
    return (int)(n < 1 ? 1 : n);
}
struct EqMonitorWs { unsigned* counter; double* partial; };
static EqMonitorWs eq_monitor_carve(Carver& c, int B, int K) {
    unsigned* counter = c.take<unsigned>(1);
    return EqMonitorWs{counter, c.take<double>((size_t)eq_monitor_blocks(B, K))};
}
static EqMonitorArgs eq_monitor_args(const dccn_eq_monitor& m) {
    EqMonitorArgs a{};
    a.chest = m.chest; a.chan = m.chan; a.gt_per_symbol = m.chan_per_symbol ? 1 : 0; a.B = m.B; a.S = m.S; a.K = m.K;
    a.metrics = m.metrics; a.tx_power = m.tx_power; a.noise_power = m.noise_power; a.acc = m.acc5; a.rms_out = m.rms_out;
    Carver c(m.workspace, m.workspace_bytes);
    const EqMonitorWs w = eq_monitor_carve(c, m.B, m.K);
    a.counter = w.counter; a.partial = w.partial;
    return a;
}

// Everything a step decides, decided before its first launch: eq_step_plan checks every argument and fills this, the
// eq_issue_* functions below only read it.  A refused step has launched nothing (also inside a stream capture).
struct EqStepPlan {
    EqDims d;
    EqWs w;
    EqBnParts bnp;
    bool train;
    const dccn_receive_out* ro;     // the receive path (dccn_eq_receive_step): no labels, no metrics
    // round-3 plan (TUNE_EQ_REPLAN): merged element-wise launches, the corr / eq C-Conv pair as grouped launches with the
    // concat / split of model.py:456 in the GEMM stores, ONE job-table launch for every gradient reduction + Adam
    // TUNE_EQ_REPLAN: 0 launch-per-stage plan, 1 re-plan, 2 re-plan with every dense split-K sum as its own launch
    // (debugging), 3 re-plan without the fused pilot bottleneck (bit-identical gradients to plan 0)
    bool replan, keep_slabs, bn, pair;
    long long g_in, g_w, g_b;       // the pair's strides: eq -> corr tensors, conv3d_3 (eq) -> conv3d_2 (corr) kernels / biases
    bool rides;                     // `input:0` is the single-pass kernel's (eq_norm_rides_ok)
    bool pre;                       // the previous step ran it for this batch on its optimizer launch (x_prenormalised)
    int nslot;
    // the next batch's generator as a rider of this step (dccn_eq_buffers.gen_next_rides): on the bottleneck backward launch
    // when the plan has it and the descriptor has no Doppler frames (ga: its argument block), else as the step's first launch
    // (same batch either way); gsc: every chain's (nbits, offset, seed) for either launch (n == 0: one chain)
    bool gen_wanted, gen_rides;
    GenStaticArgs ga;
    GenChainScalars gsc;
    bool want_snr;
    // the frozen receiver: its layout and its linear part as this step runs it (input rows, weights, bias, k extent)
    dccn_rx_shape rsh;
    RxLayout L;
    bool few_rx, folded;
    const float *rxA, *rxW, *rxb;
    int rxK;
    bool fin_deferred;              // training: the tail's metric reduction rides on the optimizer launch
    // the tail is the one stage whose kernels depend on the modulation: the chains of a group run it class by class -- one
    // launch (pair) per distinct nbits, carrying the chains cls[c] of that modulation -- everything else is one launch for
    // all of them.  fin_class: the metric reduction each chain's optimizer-launch job runs.
    int n_class, fin_class[kMaxChains], cls_nbits[4];
    bool cls_fused[4];              // dense + tail (or + decision) in one launch, else dense and then a stand-alone kernel
    ChainCtx cls[4];
    // `input:0` of the next batch on the optimizer launch: x_next, or (y, noise, partials) of the fused generator (nv)
    bool next_rides;
    const float* rin;
    NormVirtual nv;
    bool has_mon;                   // the training loop's per-step monitors on the optimizer launch (dccn_eq_buffers.monitor)
    EqMonitorArgs mon;
};
// what one phase of the step leaves for the next: where the launches put their partial results, and which element-wise
// stages the GEMMs took onto their stores
struct EqStepCarry {
    PowerPartials pp;
    TailFinalizeArgs fin[4];
    bool snr_pending;               // the pilot monitor runs on the optimizer launch
    DeferredSlabs ds5, dsT, ds4, ds3, ds2, ds1, ds0;        // (null slabs: the gradient arena holds the result)
    FoldDefer fpair[2], fconv;
    bool rode_T, rode[2];           // the smoothing kernel's fold / dense_4 / dense_3 were updated by riders of the bottleneck backward
};

// launches nothing
static int eq_step_plan(const dccn_eq_shape* sh, const dccn_eq_buffers* b, bool train, const dccn_receive_out* ro,
                        EqStepPlan* plan) {
    if (!b->x || (!ro && !b->bits) || !b->eq_params || !b->rx_params || !b->out_eq || !b->chest || (!ro && !b->metrics))
        return DCCN_ERR_INVALID_ARG;
    if (ro && (train || !ro->packed)) return DCCN_ERR_INVALID_ARG;
    if (train && (!b->eq_grads || !b->adam_m || !b->adam_v || !b->adam)) return DCCN_ERR_INVALID_ARG;
    EqStepPlan& p = *plan;
    p = EqStepPlan{};
    const EqDims& d = p.d = eq_dims(sh);
    Carver c(b->workspace, b->workspace_bytes);
    eq_carve(c, d, train, p.w);
    if (!b->workspace || b->workspace_bytes < align_up(c.off, 256)) return DCCN_ERR_WORKSPACE;
    const EqWs& w = p.w;
    const float *P = b->eq_params, *Q = b->rx_params;
    const int B = d.B, ncols = d.S * 2 * d.nsc;
    p.train = train; p.ro = ro;
    const int knob = g_tune[TUNE_EQ_REPLAN];
    p.replan = knob != 0; p.keep_slabs = knob == 1 || knob == 3;
    p.bn = eq_bn_ok(d, w.y, P + d.o[4], P + d.o[6], w.d1);
    if (train) p.bnp = eq_bn_parts(w.bn_part, B, d.SK2, d.Pp);
    p.g_in = w.corr - w.eq; p.g_w = d.o[14] - d.o[16]; p.g_b = d.o[15] - d.o[17];
    p.pair = p.replan && cconv_pair_ok(w.eq, P + d.o[16], w.cat, d.R, d.K, d.K, p.g_in, p.g_w, 2) && aligned16(w.corr) &&
             (p.g_b % 2 == 0);
    const dccn_gen_static* gv = b->x_next_virtual;
    p.gen_wanted = train && b->gen_next_rides != 0;
    if (p.gen_wanted && gv == nullptr) return DCCN_ERR_INVALID_ARG;
    // (the bottleneck backward launch carries the static generator body of the long prefix only: a descriptor with Doppler
    // frames or with the short prefix is the step's first launch, with the chain scalars of a group)
    p.gen_rides = p.gen_wanted && p.bn && gen_static_ok(gv) && !gen_static_doppler(gv) && gv->CP == 16;
    if (p.gen_wanted) DCCN_TRY(gen_static_args(gv, &p.ga));
    if (p.gen_wanted && tl_chain.G > 1) {
        p.gsc.n = tl_chain.G;
        for (int g = 0; g < tl_chain.G; ++g) {
            p.gsc.nbits[g] = tl_chain.gen_nbits[g]; p.gsc.offset[g] = tl_chain.gen_offset[g]; p.gsc.seed[g] = tl_chain.gen_seed[g];
        }
    }
    p.rides = eq_norm_rides_ok(d, train, b->x, w.x_norm);
    p.pre = p.rides && b->x_prenormalised != 0;
    if (b->x_prenormalised != 0 && !p.pre) return DCCN_ERR_INVALID_ARG;
    p.nslot = b->norm_slot ? 1 : 0;
    p.want_snr = b->snr_db && b->pilot_carriers && sh->P > 0;
    p.rsh = eq_rx_shape(d, sh->nbits);
    const RxLayout& L = p.L = rx_layout(&p.rsh);
    const float* Mf = b->rx_folded;
    p.few_rx = eq_few_rx_ok(d, L, w.fft, Q, w.z);
    p.folded = Mf != nullptr && eq_rx_folded_ok(d, p.few_rx, Mf, b->out_eq);
    p.rxA = p.folded ? b->out_eq : w.fft;
    p.rxW = p.folded ? Mf : Q + L.o_dense_w;
    p.rxb = p.folded ? Mf + (size_t)ncols * L.dN : Q + L.o_dense_b;
    p.rxK = p.folded ? ncols : L.dK;
    p.fin_deferred = p.replan && train;
    const ChainCtx& all = tl_chain;
    if (all.G > 1 && !(ro ? eq_receive_group_ok(eq_norm_single_ok(d, b->x, w.x_norm), p.bn, p.folded)
                          : eq_group_ok(p.rides, p.bn, p.folded)))
        return DCCN_ERR_UNSUPPORTED;
    bool done[kMaxChains] = {false, false, false, false, false, false, false, false};
    for (int g = 0; g < all.G; ++g) {
        if (done[g]) continue;
        if (p.n_class >= 4) return DCCN_ERR_INVALID_ARG;
        const int nbits = all.G == 1 ? sh->nbits : all.nbits[g];
        ChainCtx& sub = p.cls[p.n_class];
        sub = all;
        sub.G = 0;
        for (int h = g; h < all.G; ++h) {
            if (all.nbits[h] != all.nbits[g]) continue;
            sub.co.off[sub.G] = all.co.off[h]; sub.nbits[sub.G] = all.nbits[h];
            ++sub.G;
            done[h] = true;
            p.fin_class[h] = p.n_class;
        }
        p.cls_nbits[p.n_class] = nbits;
        // BPSK / QPSK: the tail rides on the few-row tiles themselves (dense_tail_impl picks the fewrow.h form for <= 96 rows)
        p.cls_fused[p.n_class] = (!p.few_rx || nbits <= 2) && dense_tail_planned(nbits, train, B, L.dN) &&
                                 dense_tail_ok(p.rxA, p.rxW, B, p.rxK, L.dN, nbits);
        ++p.n_class;
    }
    if (ro) {
        // what dense_decide_impl / decide_impl ask of the outputs; the stand-alone decision kernel reads z as float2
        // (a group: asked per chain, with that chain's own pointers and modulation)
        for (int g = 0; g < all.G; ++g) {
            const int nbits = all.G == 1 ? sh->nbits : all.nbits[g];
            const long long off = all.co.off[g];
            const float* llr = ro->llr ? reinterpret_cast<const float*>(reinterpret_cast<const char*>(ro->llr) + off) : nullptr;
            const float* prob = ro->prob ? reinterpret_cast<const float*>(reinterpret_cast<const char*>(ro->prob) + off) : nullptr;
            if (!decide_outputs_aligned(llr, prob, nbits)) return DCCN_ERR_INVALID_ARG;
            if (!(p.cls_fused[p.fin_class[g]] && nbits <= 2) && ((reinterpret_cast<uintptr_t>(w.z) + (uintptr_t)off) & 7u) != 0)
                return DCCN_ERR_INVALID_ARG;
        }
    }
    p.nv = norm_virtual_none();
    if (p.fin_deferred) {               // (the launch-per-stage plan has no optimizer launch that could carry either)
        if (gv != nullptr && (!gv->y || !gv->noise || !gv->power_partial || gv->frames != B ||
                              2 * (gv->K + gv->CP) * gv->S != ncols))
            return DCCN_ERR_INVALID_ARG;
        p.rin = gv ? gv->y : b->x_next;
        p.next_rides = p.rides && p.rin != nullptr && norm_fused_ok(p.rin, w.x_norm, B, ncols);
        if (gv != nullptr && !p.next_rides) return DCCN_ERR_INVALID_ARG;    // nothing else would form that batch: ask dccn_eq_norm_rides first
        if (gv != nullptr) p.nv = norm_virtual_gen(gv, ceil_div(gv->frames, kGenFramesPerBlock), nullptr);
        if (const dccn_eq_monitor* m = b->monitor) {
            if (!m->chan || !m->acc5 || m->chest != b->chest || m->metrics != b->metrics || m->tx_power != b->tx_power || m->B != B ||
                m->S != d.S || m->K != d.K || !m->workspace || m->workspace_bytes < dccn_eq_monitor_workspace_size(B, d.S, d.K))
                return DCCN_ERR_INVALID_ARG;
            p.mon = eq_monitor_args(*m);
            p.has_mon = true;
        }
    }
    // invariants of the step's own carve and plan: the gradients of the pair's tensors lie as far apart as the tensors, and a
    // generator that rides has the bottleneck backward launch to ride on
    if (train && p.pair && w.dcorr - w.deq != p.g_in) return DCCN_ERR_STATE;
    if (p.gen_rides && !p.bn) return DCCN_ERR_STATE;
    return DCCN_OK;
}

// the generator / R0 launch through dense_5: equalizer_ofdm (model.py:349-478)
static int eq_issue_forward(const dccn_eq_shape* sh, const dccn_eq_buffers* b, const EqStepPlan& p, dccn_adam_hparams hp,
                            hipStream_t s, EqStepCarry* k) {
    const EqDims& d = p.d;
    const EqWs& w = p.w;
    const float* P = b->eq_params;
    float* h = b->chest;
    const int B = d.B, R = d.R, K = d.K, SK2 = d.SK2, K2 = 2 * d.K, N2 = 2 * d.nsc, ncols = d.S * N2;
    const long long nBK = (long long)B * SK2;          // floats in a [B,S,K,2] tensor
    if (p.gen_wanted && !p.gen_rides) DCCN_TRY(gen_static_launch(b->x_next_virtual, s, p.gsc.n > 0 ? &p.gsc : nullptr));
    // `input:0` (ofdmreceiver_np.py:128-137) + tx_power partials
    // (training: the optimizer's per-step bookkeeping rides on this first launch)
    // pipelined: the previous step ran this launch for us on its optimizer launch (dccn_eq_buffers.x_next)
    if (p.pre) norm_power_partials(B, ncols, w.ws_norm, w.n_norm, b->x, w.x_norm, &k->pp, p.nslot);
    else DCCN_TRY(norm_impl(b->x, w.x_norm, nullptr, nullptr, !p.ro && b->tx_power != nullptr, &k->pp, B, ncols, 1e-9f, 8.0f,
                            p.train ? b->adam : nullptr, hp, w.ws_norm, w.n_norm, s, p.nslot));
    // model.py:363 layer_norm, :369 dense, :378 C-Conv "DFT"; the expansion of the :428 smoothing C-Conv (S x K, same)
    // into the block-Toeplitz matrix of a dense layer depends on the parameters only and shares the launch
    if (p.replan) {
        DCCN_LAUNCH_CHAINS_Z(eq_prep_kernel, dim3(B + ew_blocks_n((long long)SK2 * SK2)), dim3(256), 0, s, (const float*)w.x_norm,
                             w.ln, B, ncols, 1e-12f, P + d.o[12], P + d.o[13], w.T, w.be, d.S, K,
                             p.pre ? b->adam : (dccn_adam_state*)nullptr, hp);
        DCCN_LAUNCH_CHECK();
    } else {
        DCCN_NO_CHAINS();
        hipLaunchKernelGGL(layer_norm_fwd_kernel, dim3(B), dim3(256), 0, s, (const float*)w.x_norm, w.ln, (float*)nullptr,
                           (float*)nullptr, ncols, 1e-12f);
        DCCN_LAUNCH_CHECK();
    }
    DCCN_TRY(dense_fwd_impl(w.ln + d.win, P + d.o[0], P + d.o[1], w.t1, R, d.cp ? N2 : K2, K2, s, N2));
    DCCN_TRY(cconv_fwd_impl(w.t1, P + d.o[2], P + d.o[3], w.y, R, K, K, s));
    // :394-426 pilot bottleneck
    if (p.bn) {                             // both layers of the bottleneck in one launch (eq_bottleneck.h)
        DCCN_TRY(eq_bottleneck_fwd_launch(w.y, P + d.o[4], P + d.o[5], P + d.o[6], P + d.o[7], w.d1, w.d2, B, SK2, d.Pp, s));
    } else {
        DCCN_TRY(dense_fwd_impl(w.y, P + d.o[4], P + d.o[5], w.d1, B, SK2, d.Pp, s));
        DCCN_TRY(dense_fwd_impl(w.d1, P + d.o[6], P + d.o[7], w.d2, B, d.Pp, SK2, s));
    }
    DCCN_TRY(dense_fwd_impl(w.d2, P + d.o[8], P + d.o[9], w.d3, B, SK2, SK2, s));
    {
        bool fused = false;                 // tanh in the GEMM's store when the plan has the stage (few-row batches)
        DCCN_TRY(dense_fwd_impl(w.d3, P + d.o[10], P + d.o[11], w.d4, B, SK2, SK2, s, 0, 2, &fused));
        if (!fused) {
            DCCN_NO_CHAINS();
            hipLaunchKernelGGL(tanh_fwd_kernel, dim3(ew_blocks_n(nBK)), dim3(256), 0, s, (const float*)w.d4, w.d4, nBK);
            DCCN_LAUNCH_CHECK();
        }
    }
    // :428 smoothing C-Conv as a dense layer -> channel estimate
    if (!p.replan) {
        DCCN_NO_CHAINS();
        hipLaunchKernelGGL(cconv2d_same_expand_kernel, dim3(ew_blocks_n((long long)SK2 * SK2)), dim3(256), 0, s,
                           P + d.o[12], P + d.o[13], w.T, w.be, d.S, K, d.S, K);
        DCCN_LAUNCH_CHECK();
    }
    // :431-438 equalise + autocorrelation ride on the store of this GEMM when the plan has the stage; the :465-475 pilot
    // monitor then runs on the optimizer launch (training) or as its own small launch (evaluation)
    bool eq_fused = false, snr_now = false;
    if (p.replan) DCCN_TRY(dense_fwd_impl(w.d4, w.T, w.be, h, B, SK2, SK2, s, 0, 5, &eq_fused, w.y, w.eq, w.corr));
    else DCCN_TRY(dense_fwd_impl(w.d4, w.T, w.be, h, B, SK2, SK2, s));
    if (eq_fused) {
        k->snr_pending = p.want_snr && p.train;
        snr_now = p.want_snr && !p.train;
    } else if (p.replan && p.want_snr) {
        const int eb = (int)ew_blocks_n(nBK / 2);
        DCCN_NO_CHAINS();
        hipLaunchKernelGGL(equalize_fwd_snr_kernel, dim3(eb + ceil_div(B, 4)), dim3(256), 0, s, (const float2*)w.y,
                           (const float2*)h, (float2*)w.eq, (float2*)w.corr, nBK / 2, eb, b->pilot_carriers, b->snr_db, B,
                           d.S, K, sh->P);
        DCCN_LAUNCH_CHECK();
    } else {
        DCCN_NO_CHAINS();
        hipLaunchKernelGGL(equalize_fwd_kernel, dim3(ew_blocks_n(nBK / 2)), dim3(256), 0, s, (const float2*)w.y,
                           (const float2*)h, (float2*)w.eq, (float2*)w.corr, nBK / 2);
        DCCN_LAUNCH_CHECK();
        snr_now = p.want_snr;
    }
    if (snr_now) {
        DCCN_LAUNCH_CHAINS_Z(pilot_snr_kernel, dim3(B), dim3(64), 0, s, (const float2*)w.eq, b->pilot_carriers, b->snr_db, d.S, K,
                             sh->P);
        DCCN_LAUNCH_CHECK();
    }
    // :439-449 C-Conv "IDFT" of corr and eq, :456-463 concat + dense back to the receiver's input
    if (p.pair) {
        // both C-Convs in one grid; their stores interleave the two IQ-pair streams into cat = [.., K, (eq, corr)]
        DCCN_TRY(cconv_fwd_grouped_impl(w.eq, P + d.o[16], P + d.o[17], w.cat, R, K, K, 2, p.g_in, p.g_w, p.g_b, true, s));
    } else {
        DCCN_TRY(cconv_fwd_impl(w.corr, P + d.o[14], P + d.o[15], w.corc, R, K, K, s));
        DCCN_TRY(cconv_fwd_impl(w.eq, P + d.o[16], P + d.o[17], w.eqc, R, K, K, s));
        DCCN_NO_CHAINS();
        hipLaunchKernelGGL(concat_pairs_kernel, dim3(ew_blocks_n((long long)R * K)), dim3(256), 0, s, (const float2*)w.eqc,
                           (const float2*)w.corc, (float4*)w.cat, (long long)R * K);
        DCCN_LAUNCH_CHECK();
    }
    return dense_fwd_impl(w.cat, P + d.o[18], P + d.o[19], b->out_eq, R, 4 * K, N2, s);
}

// the frozen basic receiver (model.py:1222-1292) for the chains of modulation class c: + loss/BER through the tail (evaluation,
// training), or the decision stage in its place (receive: the same route, so z has the bits the evaluation step computes)
static int eq_issue_rx(const dccn_eq_buffers* b, const EqStepPlan& p, int c, hipStream_t s, EqStepCarry* k) {
    const EqWs& w = p.w;
    const RxLayout& L = p.L;
    const float* Q = b->rx_params;
    const dccn_receive_out* ro = p.ro;
    const int B = p.d.B, nbits = p.cls_nbits[c];
    const bool train = p.train;
    TailFinalizeArgs* fin = p.fin_deferred ? &k->fin[c] : nullptr;
    const ChainScope scope(p.cls[c]);
    if (!p.folded)
        DCCN_TRY(cconv_fwd_impl(b->out_eq + p.d.win, Q + L.o_conv_w, Q + L.o_conv_b, w.fft, p.d.R, p.rsh.kin, p.d.F, s, 2 * p.d.nsc));
    if (p.cls_fused[c]) {
        if (ro)
            return dense_decide_impl(p.rxA, p.rxW, p.rxb, nbits >= 3 ? w.z : nullptr, Q + L.o_tail, ro->packed, ro->llr, ro->prob, B,
                                     p.rxK, L.dN, nbits, s);
        return dense_tail_impl(train, p.rxA, p.rxW, p.rxb, nullptr, b->bits, Q + L.o_tail, b->prob, b->metrics, train ? w.dz : nullptr,
                               train ? w.dtail : nullptr, B, p.rxK, L.dN, nbits, &k->pp, b->tx_power, w.ws_tail, w.n_tail, s, fin);
    }
    DCCN_TRY(dense_fwd_impl(p.rxA, p.rxW, p.rxb, w.z, B, p.rxK, L.dN, s));
    if (ro) return decide_impl(w.z, Q + L.o_tail, ro->packed, ro->llr, ro->prob, B, p.d.D, nbits, s);
    return tail_impl(train, w.z, b->bits, Q + L.o_tail, b->prob, b->metrics, train ? w.dz : nullptr, train ? w.dtail : nullptr,
                     L.cells, nbits, &k->pp, b->tx_power, w.ws_tail, w.n_tail, s, fin);
}

// through the frozen receiver to its input, then the equaliser, last layer first
static int eq_issue_backward(const dccn_eq_buffers* b, const EqStepPlan& p, dccn_adam_hparams hp, hipStream_t s, EqStepCarry* k) {
    const EqDims& d = p.d;
    const EqWs& w = p.w;
    const RxLayout& L = p.L;
    const float *P = b->eq_params, *Q = b->rx_params;
    float* G = b->eq_grads;
    const int B = d.B, R = d.R, K = d.K, SK2 = d.SK2, K2 = 2 * d.K, N2 = 2 * d.nsc;
    const long long nBK = (long long)B * SK2;
    const bool keep_slabs = p.keep_slabs, pair = p.pair;
    if (p.folded) {
        // dout = dz . Mf^T in one GEMM (the zero rows of Mf leave zeros in the cyclic-prefix samples when cp = 0)
        DCCN_TRY(dense_bwd_x_impl(w.dz, p.rxW, w.dout, B, p.rxK, L.dN, s));
    } else {
        DCCN_TRY(dense_bwd_x_impl(w.dz, Q + L.o_dense_w, w.dfft, B, L.dK, L.dN, s));
        if (!d.cp) {                                        // nothing flows back into the cyclic-prefix samples
            DCCN_NO_CHAINS();
            hipLaunchKernelGGL(zero_fill_kernel, dim3(ew_blocks_n((long long)R * N2)), dim3(256), 0, s, w.dout,
                               (long long)R * N2);
            DCCN_LAUNCH_CHECK();
        }
        DCCN_TRY(cconv_bwd_x_impl(w.dfft, Q + L.o_conv_w, w.dout + d.win, R, p.rsh.kin, d.F, s, N2));
    }
    // replan: every weight gradient stays where its GEMM left it (finished in the gradient arena, or as split-K slabs in the
    // layer's own workspace) until the optimizer launch
    bool split_done = false;                // dcat's stores write deqc / dcorc themselves (when the plan has the stage)
    DCCN_TRY(dense_bwd_full_impl(w.cat, w.dout, P + d.o[18], w.dcat, G + d.o[18], G + d.o[19], R, 4 * K, N2,
                                 w.ws_l[EQL_DENSE5], w.n_l[EQL_DENSE5], s, 1, nullptr, nullptr, keep_slabs ? &k->ds5 : nullptr,
                                 pair ? w.deqc : nullptr, pair ? (long long)(w.dcorc - w.deqc) : 0, pair ? &split_done : nullptr));
    if (!split_done) {
        DCCN_NO_CHAINS();
        hipLaunchKernelGGL(split_pairs_kernel, dim3(ew_blocks_n((long long)R * K)), dim3(256), 0, s, (const float4*)w.dcat,
                           (float2*)w.deqc, (float2*)w.dcorc, (long long)R * K);
        DCCN_LAUNCH_CHECK();
    }
    if (pair) {
        // dX and dWeff slabs of both C-Convs in one grid (group 0 = eq, 1 = corr)
        DCCN_TRY(cconv_bwd_grouped_impl(w.eq, w.deqc, P + d.o[16], w.deq, R, K, K, 2, p.g_in, w.dcorc - w.deqc, p.g_w,
                                        w.ws_l[EQL_PAIR], w.n_l[EQL_PAIR], k->fpair, s));
    } else {
        DCCN_TRY(cconv_bwd_x_impl(w.deqc, P + d.o[16], w.deq, R, K, K, s));
        DCCN_TRY(cconv_bwd_w_impl(w.eq, w.deqc, G + d.o[16], G + d.o[17], R, K, K, w.ws_l[EQL_PAIR], w.n_l[EQL_PAIR], s));
        DCCN_TRY(cconv_bwd_x_impl(w.dcorc, P + d.o[14], w.dcorr, R, K, K, s));
        DCCN_TRY(cconv_bwd_w_impl(w.corr, w.dcorc, G + d.o[14], G + d.o[15], R, K, K, w.ws_l[EQL_PAIR], w.n_l[EQL_PAIR], s));
    }
    DCCN_LAUNCH_CHAINS_Z(equalize_bwd_kernel, dim3(ew_blocks_n(nBK / 2)), dim3(256), 0, s, (const float2*)w.y,
                         (const float2*)b->chest, (const float2*)w.deq, (const float2*)w.dcorr, (float2*)w.dy, (float2*)w.dh,
                         nBK / 2);
    DCCN_LAUNCH_CHECK();
    bool tg_fused = false;                  // tanh gradient on the dX store: dd4 = (dh . T^T) (1 - d4^2)
    DeferredSlabs& dsT = k->dsT;
    DCCN_TRY(dense_bwd_full_impl(w.d4, w.dh, w.T, w.dd4, w.dT, w.dbe, B, SK2, SK2, w.ws_l[EQL_SMOOTH], w.n_l[EQL_SMOOTH], s, 3,
                                 w.d4, &tg_fused, keep_slabs ? &dsT : nullptr));
    if (dsT.dw_slabs) {
        // the fold of this layer gathers diagonals of dT (one cache line per element): over several slabs that gather
        // thrashes the L2 (measured 53 us for the optimizer launch at 1170 frames), so the slabs are summed first
        const long long n = (long long)SK2 * SK2;
        DCCN_TRY(launch_splitk_reduce2(dsT.dw_slabs, dsT.splits, n, w.dT, n, dsT.db_slabs, (long long)SK2, w.dbe, (long long)SK2, s));
        dsT.dw_slabs = dsT.db_slabs = nullptr;
    }
    if (!p.replan) {
        DCCN_NO_CHAINS();
        hipLaunchKernelGGL(cconv2d_same_reduce_kernel, dim3(d.S * K + 1), dim3(64), 0, s, (const float*)w.dT,
                           (const float*)w.dbe, G + d.o[12], G + d.o[13], d.S, K, d.S, K);
        DCCN_LAUNCH_CHECK();
    }
    if (!tg_fused) {
        DCCN_NO_CHAINS();
        hipLaunchKernelGGL(tanh_bwd_kernel, dim3(ew_blocks_n(nBK)), dim3(256), 0, s, (const float*)w.dd4, (const float*)w.d4,
                           w.dd4, nBK);
        DCCN_LAUNCH_CHECK();
    }
    DCCN_TRY(dense_bwd_full_impl(w.d3, w.dd4, P + d.o[10], w.dd3, G + d.o[10], G + d.o[11], B, SK2, SK2, w.ws_l[EQL_DENSE4],
                                 w.n_l[EQL_DENSE4], s, 1, nullptr, nullptr, keep_slabs ? &k->ds4 : nullptr));
    DCCN_TRY(dense_bwd_full_impl(w.d2, w.dd3, P + d.o[8], w.dd2, G + d.o[8], G + d.o[9], B, SK2, SK2, w.ws_l[EQL_DENSE3],
                                 w.n_l[EQL_DENSE3], s, 1, nullptr, nullptr, keep_slabs ? &k->ds3 : nullptr));
    const float* dy_sum;
    if (p.bn) {
        // both layers' backward in one launch: dd1, the branch's input gradient added to dy, per-block partials of the
        // four weight / bias gradients (summed by the optimizer launch)
        // riders: the Adam updates of dense_3 / dense_4 (their gradients are complete in the arena, nothing from here to the
        // end of the step touches those kernels) stream behind this launch's own blocks instead of in the optimizer launch
        EqBnRiders rd = eq_bn_no_riders();
        EqRideArgs& ride = rd.ride;
        rd.hp = hp;
        if (g_tune[TUNE_EQ_RIDERS]) {
            ride.p.param = b->eq_params; ride.p.grad = G; ride.p.m = b->adam_m; ride.p.v = b->adam_v;
            ride.p.reg_coef = b->reg_coef; ride.p.state = b->adam;
            if (dsT.dw_slabs == nullptr && g_tune[TUNE_EQ_RIDERS] != 4) {
                // the smoothing kernel's fold (a gather over the diagonals of dT: latency, not bytes) goes first
                EqOptJob& J = ride.job[ride.njobs++];
                J.kind = EQJ_CONV2D_FOLD; J.block0 = ride.blocks; J.blocks = ceil_div(d.S * K + 1, 4); J.splits = 1;
                J.off = d.o[12]; J.off_b = d.o[13]; J.src = w.dT; J.src2 = w.dbe; J.slab = (long long)SK2 * SK2; J.slab2 = SK2;
                J.kin = d.S; J.F = K;
                ride.blocks += J.blocks;
                k->rode_T = true;
            }
            for (int li = 0; li < 2; ++li) {
                const int i = li == 0 ? 10 : 8;
                const DeferredSlabs& dsl = li == 0 ? k->ds4 : k->ds3;
                if (dsl.dw_slabs != nullptr || (d.sz[i] % 4) != 0) continue;
                if (g_tune[TUNE_EQ_RIDERS] == 2 + li) continue;          // 2: only dense_3 rides, 3: only dense_4
                EqOptJob& J = ride.job[ride.njobs++];
                J.kind = EQJ_SUM; J.block0 = ride.blocks; J.blocks = EqOptBuilder::stream_blocks(d.sz[i]); J.splits = 1;
                J.off = d.o[i]; J.n = d.sz[i]; J.vec = 1; J.reg_uniform = (b->reg_uniform != 0 && b->reg_coef != nullptr) ? 1 : 0;
                ride.blocks += J.blocks;
                k->rode[li] = true;
            }
        }
        // the NEXT batch's generator rides here as well (dccn_eq_buffers.gen_next_rides): its workgroups are the first grid rows
        rd.ga = p.ga; rd.gc = p.gsc;
        if (p.gen_rides) {
            rd.gen_blocks = ceil_div(p.ga.frames, kGenFramesPerBlock);
            rd.gen_smem = gen_static_smem_bytes<7, 64, 16>();
        }
        DCCN_TRY(eq_bottleneck_bwd_launch(w.dd2, w.d1, w.y, P + d.o[4], P + d.o[6], w.dy, w.dflat, p.bnp, B, SK2, d.Pp, rd, s));
        dy_sum = w.dflat;
    } else {
        DCCN_TRY(dense_bwd_full_impl(w.d1, w.dd2, P + d.o[6], w.dd1, G + d.o[6], G + d.o[7], B, d.Pp, SK2, w.ws_l[EQL_DENSE2],
                                     w.n_l[EQL_DENSE2], s, 1, nullptr, nullptr, keep_slabs ? &k->ds2 : nullptr));
        // dy += (gradient through the pilot branch): by the dX stores themselves when the launch plan has the stage (the sum
        // then lands in dflat), else by a launch of its own
        bool add_fused = false;
        DCCN_TRY(dense_bwd_full_impl(w.y, w.dd1, P + d.o[4], w.dflat, G + d.o[4], G + d.o[5], B, SK2, d.Pp, w.ws_l[EQL_DENSE1],
                                     w.n_l[EQL_DENSE1], s, 4, w.dy, &add_fused, keep_slabs ? &k->ds1 : nullptr));
        if (!add_fused) {
            DCCN_NO_CHAINS();
            hipLaunchKernelGGL(add_inplace_kernel, dim3(ew_blocks_n(nBK)), dim3(256), 0, s, w.dy, (const float*)w.dflat, nBK);
            DCCN_LAUNCH_CHECK();
        }
        dy_sum = add_fused ? w.dflat : w.dy;
    }
    const bool conv_grouped = p.replan && cconv_pair_ok(w.t1, P + d.o[2], w.dt1, R, K, K, 0, 0, 0) && aligned16(dy_sum);
    if (conv_grouped) {
        DCCN_TRY(cconv_bwd_grouped_impl(w.t1, dy_sum, P + d.o[2], w.dt1, R, K, K, 1, 0, 0, 0, w.ws_l[EQL_CONV], w.n_l[EQL_CONV],
                                        &k->fconv, s));
    } else {
        DCCN_TRY(cconv_bwd_x_impl(dy_sum, P + d.o[2], w.dt1, R, K, K, s));
        DCCN_TRY(cconv_bwd_w_impl(w.t1, dy_sum, G + d.o[2], G + d.o[3], R, K, K, w.ws_l[EQL_CONV], w.n_l[EQL_CONV], s));
    }
    return dense_bwd_w_impl(w.ln + d.win, w.dt1, G + d.o[0], G + d.o[1], R, d.cp ? N2 : K2, K2, w.ws_l[EQL_DENSE], w.n_l[EQL_DENSE], s,
                            keep_slabs ? &k->ds0 : nullptr, N2);
}

// optimizer: Equalizer/* only (ofdmreceiver_np_mp.py:330), L2 terms enter through reg_coef.  The re-plan's ONE launch walks a
// job table: every gradient reduction + Adam, `input:0` of the next batch, the monitors, the tail's metric reduction
static int eq_issue_update(const dccn_eq_shape* sh, const dccn_eq_buffers* b, const EqStepPlan& p, dccn_adam_hparams hp,
                           hipStream_t s, EqStepCarry* k) {
    const EqDims& d = p.d;
    const EqWs& w = p.w;
    const int B = d.B, K = d.K, SK2 = d.SK2, ncols = d.S * 2 * d.nsc;
    if (!p.replan)
        return adam_impl(b->eq_params, b->eq_grads, b->adam_m, b->adam_v, b->reg_coef, nullptr, b->adam, hp, d.o[20], s, false);
    EqOptBuilder ob;
    memset(&ob.a, 0, sizeof(ob.a));
    ob.a.param = b->eq_params; ob.a.grad = b->eq_grads; ob.a.m = b->adam_m; ob.a.v = b->adam_v; ob.a.reg_coef = b->reg_coef;
    ob.a.state = b->adam;
    const bool uni = b->reg_uniform != 0 && b->reg_coef != nullptr;
    if (p.next_rides) {
        // x_norm is read by the layer norm only, long before this launch
        PowerPartials pn;
        norm_power_partials(B, ncols, w.ws_norm, w.n_norm, p.rin, w.x_norm, &pn, p.nslot ^ 1);
        ob.norm_next(p.rin, w.x_norm, B, ncols, b->tx_power != nullptr ? const_cast<double*>(pn.partial) : nullptr,
                     norm_fused_blocks(ncols), p.nv);
    }
    eq_opt_dense(ob, d, 0, k->ds0, 2 * K, uni);
    const FoldDefer& fconv = k->fconv;
    if (fconv.slabs) ob.cconv_fold(d.o[2], d.o[3], fconv.slabs, fconv.colsum, fconv.splits, fconv.slab, K, K);
    else { ob.plain(d.o[2], d.sz[2]); ob.plain(d.o[3], d.sz[3]); }
    if (p.bn) {
        const EqBnParts& q = p.bnp;
        ob.slabs(d.o[4], d.sz[4], q.w1, q.tiles, (long long)SK2 * d.Pp, uni);
        ob.slabs(d.o[5], d.sz[5], q.b1, q.tiles, d.Pp, uni);
        ob.slabs(d.o[6], d.sz[6], q.w2, q.tiles, (long long)d.Pp * SK2, uni);
        ob.slabs(d.o[7], d.sz[7], q.b2, q.tiles, SK2, uni);
    } else {
        eq_opt_dense(ob, d, 4, k->ds1, d.Pp, uni);
        eq_opt_dense(ob, d, 6, k->ds2, SK2, uni);
    }
    eq_opt_dense(ob, d, 8, k->ds3, SK2, uni, k->rode[1]);
    eq_opt_dense(ob, d, 10, k->ds4, SK2, uni, k->rode[0]);
    const DeferredSlabs& dsT = k->dsT;
    if (!k->rode_T)
        ob.conv2d_fold(d.o[12], d.o[13], dsT.dw_slabs ? dsT.dw_slabs : w.dT, (dsT.dw_slabs && dsT.db_slabs) ? dsT.db_slabs : w.dbe,
                       dsT.dw_slabs ? dsT.splits : 1, (long long)SK2 * SK2, SK2, d.S, K);
    for (int g = 1; g >= 0; --g) {          // arena order: conv3d_2 (corr, group 1), then conv3d_3 (eq, group 0)
        const int i = g == 1 ? 14 : 16;
        const FoldDefer& f = k->fpair[g];
        if (f.slabs) ob.cconv_fold(d.o[i], d.o[i + 1], f.slabs, f.colsum, f.splits, f.slab, K, K);
        else { ob.plain(d.o[i], d.sz[i]); ob.plain(d.o[i + 1], d.sz[i + 1]); }
    }
    eq_opt_dense(ob, d, 18, k->ds5, 2 * d.nsc, uni);
    if (p.has_mon) {
        ob.monitor(p.mon, eq_monitor_blocks(B, K));
        for (int c = 0; c < p.n_class; ++c) { k->fin[c].mon_acc = p.mon.acc; k->fin[c].mon_noise = p.mon.noise_power; }
    }
    ob.tail_finalize(k->fin, p.n_class, p.fin_class);
    if (k->snr_pending) ob.pilot_snr(w.eq, b->pilot_carriers, b->snr_db, B, d.S, K, sh->P);
    return launch_eq_opt(ob, hp, s);
}

// ro != nullptr: the receive path (dccn_eq_receive_step): the evaluation step's forward with the tail section replaced by the
// decision stage (decide.h) -- no labels, no metrics; bits / metrics / prob / tx_power of `b` are not touched
static int eq_step_impl(const dccn_eq_shape* sh, const dccn_eq_buffers* b, bool train, dccn_adam_hparams hp,
                        hipStream_t s, const dccn_receive_out* ro = nullptr) {
    if (!eq_shape_ok(sh) || !b) return DCCN_ERR_INVALID_ARG;
    const TuneScope tune(b->tuning);
    EqStepPlan plan;
    DCCN_TRY(eq_step_plan(sh, b, train, ro, &plan));
    EqStepCarry k{};
    DCCN_TRY(eq_issue_forward(sh, b, plan, hp, s, &k));
    for (int c = 0; c < plan.n_class; ++c) DCCN_TRY(eq_issue_rx(b, plan, c, s, &k));
    if (!train) return DCCN_OK;
    DCCN_TRY(eq_issue_backward(b, plan, hp, s, &k));
    return eq_issue_update(sh, b, plan, hp, s, &k);
}
