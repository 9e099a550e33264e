// libdccn.so -- the equaliser: fused step, chain groups, stage operators, monitors (see abi_impl.h for how the library is cut into units)
#include "abi_impl.h"

namespace dccn {
#include "eq_step.h"
}  // namespace dccn

using namespace dccn;

extern "C" {

// ---- fused equaliser step ---------------------------------------------------------------------------
int dccn_eq_param_offsets(const dccn_eq_shape* shape, long long* offsets) {
    if (!eq_shape_ok(shape) || !offsets) return DCCN_ERR_INVALID_ARG;
    const EqDims d = eq_dims(shape);
    for (int i = 0; i < 21; ++i) offsets[i] = d.o[i];
    return DCCN_OK;
}
size_t dccn_eq_workspace_size(const dccn_eq_shape* shape, int train) {
    if (!eq_shape_ok(shape)) return 0;
    return eq_ws_bytes(shape, train);
}
int dccn_eq_workspace_tensor(const dccn_eq_shape* shape, int train, const char* name, size_t* byte_offset, size_t* count) {
    if (!eq_shape_ok(shape) || !name || !byte_offset || !count) return DCCN_ERR_INVALID_ARG;
    int status = DCCN_ERR_INVALID_ARG;          // (an unknown name; a training-only tensor of an evaluation workspace is not carved)
    Carver c(nullptr, 0);
    EqWs w;
    eq_carve(c, eq_dims(shape), train != 0, w, [&](const EqWsTensor& t, size_t off, size_t n) {
        if (t.name == nullptr || strcmp(t.name, name) != 0) return;
        *byte_offset = off;
        *count = n;
        status = DCCN_OK;
    });
    return status;
}
size_t dccn_eq_rx_folded_floats(const dccn_eq_shape* shape) {
    if (!eq_shape_ok(shape)) return 0;
    const size_t N2 = 2 * (size_t)(shape->K + shape->CP), dN = 2 * (size_t)shape->D;
    return (size_t)shape->S * N2 * dN + dN;
}
int dccn_eq_rx_fold(const dccn_eq_shape* shape, const float* rx_params, float* out, dccn_stream_t stream) {
    if (!eq_shape_ok(shape) || !rx_params || !out) return DCCN_ERR_INVALID_ARG;
    const EqDims d = eq_dims(shape);
    const dccn_rx_shape rsh = eq_rx_shape(d, shape->nbits);
    const RxLayout L = rx_layout(&rsh);
    const int N2 = 2 * d.nsc, rows = d.S * N2;
    hipLaunchKernelGGL(eq_rx_fold_kernel, dim3(rows + 1), dim3(256), 0, (hipStream_t)stream, rx_params + L.o_conv_w,
                       rx_params + L.o_conv_b, rx_params + L.o_dense_w, rx_params + L.o_dense_b, out, out + (size_t)rows * L.dN,
                       d.S, N2, d.win, rsh.kin, d.F, L.dN);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}
int dccn_eq_eval_step(const dccn_eq_shape* shape, const dccn_eq_buffers* buf, dccn_stream_t stream) {
    return eq_step_impl(shape, buf, false, dccn_adam_hparams(), (hipStream_t)stream);
}
int dccn_eq_receive_step(const dccn_eq_shape* shape, const dccn_eq_buffers* buf, const dccn_receive_out* out,
                         dccn_stream_t stream) {
    if (!out || !out->packed) return DCCN_ERR_INVALID_ARG;
    return eq_step_impl(shape, buf, false, dccn_adam_hparams(), (hipStream_t)stream, out);
}
int dccn_eq_train_step(const dccn_eq_shape* shape, const dccn_eq_buffers* buf, dccn_adam_hparams hp,
                       dccn_stream_t stream) {
    return eq_step_impl(shape, buf, true, hp, (hipStream_t)stream);
}
}  // extern "C"

// ---- chain groups: G independent equaliser chains per launch sequence (common.h ChainCtx) ------------------------------
// every device pointer of chain g must lie at ONE byte offset from chain 0's (the chains' arenas have the same layout).
// Each struct's device-pointer fields are listed ONCE, by a function that hands them to a PtrList in a fixed order; where an entry
// point holds only some of them to the contract, that subset is a list of its own which the full list starts with.
struct PtrList {
    const void* p[32];
    int n = 0;
    bool ok = true;
    void operator()(const void* q) {
        if (n < 32) p[n++] = q;
        else ok = false;
    }
};
// what the forward-only step reads or writes (dccn_eq_receive_step: labels, metrics, gradients and optimizer state are not touched)
static void eq_buffers_forward_pointers(const dccn_eq_buffers& b, PtrList& f) {
    f(b.x); f(b.eq_params); f(b.rx_params); f(b.rx_folded); f(b.out_eq); f(b.chest); f(b.snr_db); f(b.pilot_carriers); f(b.workspace);
}
// (prob is no part of the arena -- its size depends on the modulation -- and a training group refuses it)
static void eq_buffers_pointers(const dccn_eq_buffers& b, PtrList& f) {
    eq_buffers_forward_pointers(b, f);
    f(b.bits); f(b.eq_grads); f(b.adam_m); f(b.adam_v); f(b.reg_coef); f(b.adam); f(b.metrics); f(b.tx_power); f(b.x_next);
}
static void receive_out_pointers(const dccn_receive_out& o, PtrList& f) { f(o.packed); f(o.llr); f(o.prob); }
static void eq_monitor_pointers(const dccn_eq_monitor& m, PtrList& f) {
    f(m.chest); f(m.chan); f(m.metrics); f(m.tx_power); f(m.noise_power); f(m.acc5); f(m.rms_out); f(m.workspace);
}
// what the normalisation of the next batch reads from a descriptor (dccn_eq_buffers.x_next_virtual)
static void gen_static_norm_pointers(const dccn_gen_static& g, PtrList& f) {
    f(g.y); f(g.noise); f(g.power_partial); f(g.noise_partial); f(g.noise_power_out);
}
static void gen_static_pointers(const dccn_gen_static& g, PtrList& f) {
    gen_static_norm_pointers(g, f);
    f(g.bits_out); f(g.cell_map); f(g.const_tab); f(g.idft); f(g.coeff); f(g.alpha); f(g.snr_db); f(g.tx_out); f(g.H_out);
    for (int i = 0; i < g.n_profiles; ++i) { f(g.profiles[i].coeff); f(g.profiles[i].alpha); }
}

struct ChainOffsetCheck {
    long long off[kMaxChains];
    bool have[kMaxChains];
    bool ok = true;
    int n;
    explicit ChainOffsetCheck(int n_) : n(n_) { for (int g = 0; g < kMaxChains; ++g) { off[g] = 0; have[g] = false; } }
    // pointers p[g] (field f of every chain's struct)
    void field(const void* const* p) {
        for (int g = 0; g < n && ok; ++g) {
            if ((p[g] == nullptr) != (p[0] == nullptr)) { ok = false; return; }
            if (p[g] == nullptr) continue;
            const long long d = (long long)(reinterpret_cast<const char*>(p[g]) - reinterpret_cast<const char*>(p[0]));
            if (!have[g]) { off[g] = d; have[g] = true; }
            else if (off[g] != d) ok = false;
        }
    }
    // every field `list` names, of the chains' structs s[g]
    template <typename T>
    void fields(const T* const* s, void (*list)(const T&, PtrList&)) {
        PtrList v[kMaxChains];
        for (int g = 0; g < n; ++g) {
            list(*s[g], v[g]);
            if (!v[g].ok || v[g].n != v[0].n) { ok = false; return; }
        }
        for (int f = 0; f < v[0].n; ++f) {
            const void* p[kMaxChains];
            for (int g = 0; g < n; ++g) p[g] = v[g].p[f];
            field(p);
        }
    }
    bool finish(ChainCtx* ctx) {
        if (!ok) return false;
        ctx->G = n;
        for (int g = 0; g < kMaxChains; ++g) { ctx->co.off[g] = 0; ctx->nbits[g] = 0; }
        for (int g = 0; g < n; ++g) {
            if (!have[g] || (off[g] & 255) != 0 || (g > 0 && off[g] == 0)) return false;
            ctx->co.off[g] = off[g];
        }
        return true;
    }
};

// What every grouped entry point does, in this order; the callables are what is the entry point's own:
//   the count and the tables are there                                                      else DCCN_ERR_INVALID_ARG
//   valid(i)       chain i's structs are there, valid, and of chain 0's launch plan         else DCCN_ERR_INVALID_ARG
//   solo()         n_chains == 1 is the single-chain entry
//   supported()    the launches can carry a chain index (asked under the global knobs)      else DCCN_ERR_UNSUPPORTED
//   fields(chk)    the pointer lists under the layout contract; false: a refusal of its own  else DCCN_ERR_INVALID_ARG
//   scalars(ctx)   what is checked once the offsets stand, and the per-chain scalars; returns a status
//   issue()        the single-chain launch sequence on chain 0's structs, inside the group's ChainScope
template <typename Valid, typename Solo, typename Supported, typename Fields, typename Scalars, typename Issue>
static int chain_group_call(int n_chains, bool tables, Valid valid, Solo solo, Supported supported, Fields fields, Scalars scalars,
                            Issue issue) {
    if (n_chains < 1 || n_chains > kMaxChains || !tables) return DCCN_ERR_INVALID_ARG;
    for (int i = 0; i < n_chains; ++i)
        if (!valid(i)) return DCCN_ERR_INVALID_ARG;
    if (n_chains == 1) return solo();
    if (!supported()) return DCCN_ERR_UNSUPPORTED;
    ChainOffsetCheck chk(n_chains);
    ChainCtx ctx;
    if (!fields(chk) || !chk.finish(&ctx)) return DCCN_ERR_INVALID_ARG;
    DCCN_TRY(scalars(ctx));
    ChainScope scope(ctx);
    return issue();
}
static bool group_always() { return true; }
static int group_no_scalars(ChainCtx&) { return DCCN_OK; }

static bool gen_static_same_plan(const dccn_gen_static* a, const dccn_gen_static* b) {
    if (a->frames != b->frames || a->S != b->S || a->K != b->K || a->CP != b->CP || a->D != b->D || a->n_taps != b->n_taps ||
        a->L != b->L || a->identity != b->identity || a->n_profiles != b->n_profiles || a->tap_stride != b->tap_stride ||
        a->h_rep != b->h_rep || a->pilot_re != b->pilot_re || a->pilot_im != b->pilot_im ||
        a->doppler_period != b->doppler_period || a->t_sym != b->t_sym || a->Fd != b->Fd)
        return false;
    for (int i = 0; i < a->n_profiles; ++i)
        if (a->profiles[i].n_taps != b->profiles[i].n_taps || a->profiles[i].L != b->profiles[i].L ||
            a->profiles[i].identity != b->profiles[i].identity || a->profiles[i].Fd != b->profiles[i].Fd)
            return false;
    return true;
}
// one launch plan: everything but the modulation agrees
static bool eq_shapes_one_plan(const dccn_eq_shape* a, const dccn_eq_shape* c) {
    return a->batch == c->batch && a->S == c->S && a->K == c->K && a->CP == c->CP && a->cp == c->cp && a->F == c->F && a->D == c->D &&
           a->pilot_size == c->pilot_size && a->P == c->P;
}
static bool eq_monitors_one_plan(const dccn_eq_monitor* a, const dccn_eq_monitor* b) {
    return a->chan_per_symbol == b->chan_per_symbol && a->B == b->B && a->S == b->S && a->K == b->K &&
           a->workspace_bytes == b->workspace_bytes;
}
// the step's own predicates, given 16-byte aligned buffers (and rx_folded): 1 exactly where a grouped training step / a grouped
// receive step is accepted
static int eq_group_query(const dccn_eq_shape* shape, bool receive) {
    if (!eq_shape_ok(shape)) return 0;
    const EqDims d = eq_dims(shape);
    const dccn_rx_shape rsh = eq_rx_shape(d, shape->nbits);
    const RxLayout L = rx_layout(&rsh);
    const bool bn = eq_bn_ok(d, nullptr, nullptr, nullptr, nullptr);
    const bool folded = eq_rx_folded_ok(d, eq_few_rx_ok(d, L, nullptr, nullptr, nullptr), nullptr, nullptr);
    return (receive ? eq_receive_group_ok(eq_norm_single_ok(d, nullptr, nullptr), bn, folded)
                    : eq_group_ok(eq_norm_rides_ok(d, true, nullptr, nullptr), bn, folded)) ? 1 : 0;
}
// the monitors' own launch (the step's optimizer launch carries the same argument block: eq_step_plan)
static int eq_monitor_accumulate(const dccn_eq_monitor& m, hipStream_t s) {
    if (!m.chest || !m.chan || m.B <= 0 || m.S <= 0 || m.K <= 0 || (m.acc5 && !m.metrics) || (!m.acc5 && !m.rms_out))
        return DCCN_ERR_INVALID_ARG;
    if (!m.workspace || m.workspace_bytes < dccn_eq_monitor_workspace_size(m.B, m.S, m.K)) return DCCN_ERR_WORKSPACE;
    DCCN_LAUNCH_CHAINS_Z(eq_monitor_kernel, dim3(eq_monitor_blocks(m.B, m.K)), dim3(256), 0, s, eq_monitor_args(m));
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

extern "C" {

int dccn_chain_group_max(void) { return kMaxChains; }

int dccn_gen_static_frames_grouped(int n_chains, const dccn_gen_static* const* g, dccn_stream_t stream) {
    GenChainScalars gc;
    memset(&gc, 0, sizeof(gc));
    return chain_group_call(
        n_chains, g != nullptr, [&](int i) { return g[i] && gen_static_ok(g[i]) && gen_static_same_plan(g[0], g[i]); },
        [&] { return gen_static_launch(g[0], (hipStream_t)stream); }, group_always,
        [&](ChainOffsetCheck& chk) { chk.fields(g, gen_static_pointers); return true; },
        [&](ChainCtx& ctx) -> int {
            gc.n = n_chains;
            for (int i = 0; i < n_chains; ++i) { gc.nbits[i] = g[i]->nbits; gc.offset[i] = g[i]->offset; gc.seed[i] = g[i]->seed; ctx.nbits[i] = g[i]->nbits; }
            return DCCN_OK;
        },
        [&] { return gen_static_launch(g[0], (hipStream_t)stream, &gc); });
}

int dccn_gen_static_apply_grouped(int n_chains, const dccn_gen_static* const* g, float* const* x_out, float* const* noise_power,
                                  dccn_stream_t stream) {
    const auto apply = [&] { return dccn_gen_static_apply(g[0], x_out[0], noise_power ? noise_power[0] : nullptr, stream); };
    return chain_group_call(
        n_chains, g && x_out, [&](int i) { return g[i] && x_out[i] && gen_static_ok(g[i]) && gen_static_same_plan(g[0], g[i]); }, apply,
        group_always,
        [&](ChainOffsetCheck& chk) {
            chk.fields(g, gen_static_pointers);
            chk.field(reinterpret_cast<const void* const*>(x_out));
            if (noise_power) chk.field(reinterpret_cast<const void* const*>(noise_power));
            return true;
        },
        group_no_scalars, apply);
}

int dccn_eq_group_supported(const dccn_eq_shape* shape) { return eq_group_query(shape, false); }

int dccn_eq_train_step_grouped(int n_chains, const dccn_eq_shape* const* shapes, const dccn_eq_buffers* const* bufs,
                               dccn_adam_hparams hp, dccn_stream_t stream) {
    const auto step = [&] { return eq_step_impl(shapes[0], bufs[0], true, hp, (hipStream_t)stream); };
    return chain_group_call(
        n_chains, shapes && bufs,
        [&](int i) {
            if (!shapes[i] || !bufs[i] || !eq_shape_ok(shapes[i]) || !eq_shapes_one_plan(shapes[0], shapes[i])) return false;
            const dccn_eq_buffers *p = bufs[0], *q = bufs[i];
            return p->workspace_bytes == q->workspace_bytes && p->reg_uniform == q->reg_uniform &&
                   p->x_prenormalised == q->x_prenormalised && p->norm_slot == q->norm_slot &&
                   (p->x_next_virtual == nullptr) == (q->x_next_virtual == nullptr) && q->prob == nullptr;
        },
        step, [&] { return dccn_eq_group_supported(shapes[0]) != 0; },
        [&](ChainOffsetCheck& chk) {
            chk.fields(bufs, eq_buffers_pointers);
            if (bufs[0]->x_next_virtual != nullptr) {
                const dccn_gen_static* gv[kMaxChains];
                for (int i = 0; i < n_chains; ++i) {
                    gv[i] = bufs[i]->x_next_virtual;
                    if (!gen_static_same_plan(gv[0], gv[i])) return false;
                }
                // a descriptor the step arms itself (gen_next_rides: its generator runs inside the step) is held to the contract
                // whole, one that the caller's own launch filled in what the step reads of it
                chk.fields(gv, bufs[0]->gen_next_rides ? gen_static_pointers : gen_static_norm_pointers);
            }
            const dccn_eq_monitor* mm[kMaxChains];
            for (int i = 0; i < n_chains; ++i)
                if (((mm[i] = bufs[i]->monitor) == nullptr) != (mm[0] == nullptr)) return false;
            if (mm[0] == nullptr) return true;
            for (int i = 0; i < n_chains; ++i)
                if (!eq_monitors_one_plan(mm[0], mm[i])) return false;
            chk.fields(mm, eq_monitor_pointers);
            return true;
        },
        [&](ChainCtx& ctx) -> int {
            if (bufs[0]->rx_folded == nullptr) return DCCN_ERR_UNSUPPORTED;
            for (int i = 0; i < n_chains; ++i) {
                ctx.nbits[i] = shapes[i]->nbits;
                if (bufs[i]->gen_next_rides != bufs[0]->gen_next_rides) return DCCN_ERR_INVALID_ARG;
                if (bufs[0]->gen_next_rides) {                     // (the generator's per-chain scalars travel with the group)
                    const dccn_gen_static* gv = bufs[i]->x_next_virtual;
                    if (!gv) return DCCN_ERR_INVALID_ARG;
                    ctx.gen_seed[i] = gv->seed; ctx.gen_offset[i] = gv->offset; ctx.gen_nbits[i] = gv->nbits;
                }
            }
            return DCCN_OK;
        },
        step);
}

int dccn_eq_receive_group_supported(const dccn_eq_shape* shape) { return eq_group_query(shape, true); }

int dccn_eq_receive_step_grouped(int n_chains, const dccn_eq_shape* const* shapes, const dccn_eq_buffers* const* bufs,
                                 const dccn_receive_out* const* outs, dccn_stream_t stream) {
    return chain_group_call(
        n_chains, shapes && bufs && outs,
        [&](int i) {
            if (!shapes[i] || !bufs[i] || !outs[i] || !outs[i]->packed || !eq_shape_ok(shapes[i]) ||
                !eq_shapes_one_plan(shapes[0], shapes[i]))
                return false;
            const dccn_eq_buffers *p = bufs[0], *q = bufs[i];
            return p->workspace_bytes == q->workspace_bytes && p->norm_slot == q->norm_slot && q->x_prenormalised == 0;
        },
        [&] { return dccn_eq_receive_step(shapes[0], bufs[0], outs[0], stream); },
        [&] { return dccn_eq_receive_group_supported(shapes[0]) != 0; },
        [&](ChainOffsetCheck& chk) {
            chk.fields(bufs, eq_buffers_forward_pointers);
            chk.fields(outs, receive_out_pointers);
            return true;
        },
        [&](ChainCtx& ctx) -> int {
            if (bufs[0]->rx_folded == nullptr) return DCCN_ERR_INVALID_ARG;
            for (int i = 0; i < n_chains; ++i) ctx.nbits[i] = shapes[i]->nbits;
            return DCCN_OK;
        },
        [&] { return eq_step_impl(shapes[0], bufs[0], false, dccn_adam_hparams(), (hipStream_t)stream, outs[0]); });
}

int dccn_eq_monitor_accumulate_grouped(int n_chains, const dccn_eq_monitor* const* m, dccn_stream_t stream) {
    const auto accumulate = [&] { return eq_monitor_accumulate(*m[0], (hipStream_t)stream); };
    return chain_group_call(
        n_chains, m != nullptr, [&](int i) { return m[i] && eq_monitors_one_plan(m[0], m[i]); }, accumulate, group_always,
        [&](ChainOffsetCheck& chk) { chk.fields(m, eq_monitor_pointers); return true; }, group_no_scalars, accumulate);
}

int dccn_eq_norm_rides(const dccn_eq_shape* shape) {
    if (!eq_shape_ok(shape)) return 0;
    return eq_norm_rides_ok(eq_dims(shape), true, nullptr, nullptr) ? 1 : 0;
}
int dccn_eq_graph_create(const dccn_eq_shape* shape, const dccn_eq_buffers* buf, int mode, dccn_adam_hparams hp,
                         dccn_stream_t stream, dccn_rx_graph** out) {
    if (!out || !eq_shape_ok(shape) || !buf) return DCCN_ERR_INVALID_ARG;
    (void)stream;
    return graph_capture(false, out, [&](const dccn_rx_graph& g) { return eq_step_impl(shape, buf, (mode & 1) != 0, hp, g.cap); });
}

int dccn_rx_graph_launch(dccn_rx_graph* g, dccn_stream_t stream) {
    if (!g || !g->exec) return DCCN_ERR_STATE;
    DCCN_HIP(hipGraphLaunch(g->exec, (hipStream_t)stream));
    return DCCN_OK;
}
int dccn_rx_graph_destroy(dccn_rx_graph* g) {
    if (!g) return DCCN_OK;
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    if (g->ev_fork) (void)hipEventDestroy(g->ev_fork);
    if (g->ev_join) (void)hipEventDestroy(g->ev_join);
    if (g->side) (void)hipStreamDestroy(g->side);
    if (g->cap) (void)hipStreamDestroy(g->cap);
    delete g;
    return DCCN_OK;
}

int dccn_stream_synchronize(dccn_stream_t stream) {
    DCCN_HIP(hipStreamSynchronize((hipStream_t)stream));
    return DCCN_OK;
}

// ---- equaliser stage operators ------------------------------------------------------------------
static inline unsigned ew_blocks(long long n) { return ew_blocks_n(n); }
int dccn_layer_norm_fwd(const float* x, float* y, float* mean, float* inv, int rows, int cols, float eps,
                        dccn_stream_t stream) {
    if (!x || !y || rows <= 0 || cols <= 0) return DCCN_ERR_INVALID_ARG;
    hipLaunchKernelGGL(layer_norm_fwd_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, x, y, mean, inv, cols,
                       eps);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}
int dccn_layer_norm_bwd(const float* dy, const float* y, const float* inv, float* dx, int rows, int cols,
                        dccn_stream_t stream) {
    if (!dy || !y || !inv || !dx || rows <= 0 || cols <= 0) return DCCN_ERR_INVALID_ARG;
    hipLaunchKernelGGL(layer_norm_bwd_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, dy, y, inv, dx, cols);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}
int dccn_tanh_fwd(const float* x, float* y, long long n, dccn_stream_t stream) {
    if (!x || !y || n <= 0) return DCCN_ERR_INVALID_ARG;
    hipLaunchKernelGGL(tanh_fwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, y, n);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}
int dccn_tanh_bwd(const float* dy, const float* y, float* dx, long long n, dccn_stream_t stream) {
    if (!dy || !y || !dx || n <= 0) return DCCN_ERR_INVALID_ARG;
    hipLaunchKernelGGL(tanh_bwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, dy, y, dx, n);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}
int dccn_equalize_fwd(const float* y, const float* h, float* eq, float* corr, long long n_pairs,
                      dccn_stream_t stream) {
    if (!y || !h || !eq || n_pairs <= 0) return DCCN_ERR_INVALID_ARG;
    hipLaunchKernelGGL(equalize_fwd_kernel, dim3(ew_blocks(n_pairs)), dim3(256), 0, (hipStream_t)stream,
                       (const float2*)y, (const float2*)h, (float2*)eq, (float2*)corr, n_pairs);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}
int dccn_equalize_bwd(const float* y, const float* h, const float* d_eq, const float* d_corr, float* dy, float* dh,
                      long long n_pairs, dccn_stream_t stream) {
    if (!y || !h || (!d_eq && !d_corr) || (!dy && !dh) || n_pairs <= 0) return DCCN_ERR_INVALID_ARG;
    DCCN_LAUNCH_CHAINS_Z(equalize_bwd_kernel, dim3(ew_blocks(n_pairs)), dim3(256), 0, (hipStream_t)stream,
                         (const float2*)y, (const float2*)h, (const float2*)d_eq, (const float2*)d_corr, (float2*)dy,
                         (float2*)dh, n_pairs);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}
int dccn_pilot_snr(const float* eq, const int* carriers, float* snr_db, int frames, int S, int K, int P,
                   dccn_stream_t stream) {
    if (!eq || !carriers || !snr_db || frames <= 0 || S <= 0 || K <= 0 || P <= 0) return DCCN_ERR_INVALID_ARG;
    DCCN_LAUNCH_CHAINS_Z(pilot_snr_kernel, dim3(frames), dim3(64), 0, (hipStream_t)stream, (const float2*)eq, carriers,
                         snr_db, S, K, P);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}
int dccn_cconv2d_same_expand(const float* w, const float* bias, float* T, float* bias_eff, int L, int W, int kL,
                             int kW, dccn_stream_t stream) {
    if (!w || !T || L <= 0 || W <= 0 || kL <= 0 || kW <= 0) return DCCN_ERR_INVALID_ARG;
    const long long n = (long long)L * W * 2;
    if (n * n > (1LL << 31)) return DCCN_ERR_INVALID_ARG;
    hipLaunchKernelGGL(cconv2d_same_expand_kernel, dim3(ew_blocks(n * n)), dim3(256), 0, (hipStream_t)stream, w, bias,
                       T, bias_eff, L, W, kL, kW);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}
int dccn_cconv2d_same_reduce(const float* dT, const float* dbias_eff, float* dw, float* dbias, int L, int W, int kL,
                             int kW, dccn_stream_t stream) {
    if (!dT || !dw || L <= 0 || W <= 0 || kL <= 0 || kW <= 0) return DCCN_ERR_INVALID_ARG;
    hipLaunchKernelGGL(cconv2d_same_reduce_kernel, dim3(kL * kW + 1), dim3(64), 0, (hipStream_t)stream, dT, dbias_eff,
                       dw, dbias, L, W, kL, kW);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

// ---- per-step monitors of the equaliser harness in one launch (equalizer.h eq_monitor_kernel; eq_step.h eq_monitor_args) --------
size_t dccn_eq_monitor_workspace_size(int B, int S, int K) {
    if (B <= 0 || S <= 0 || K <= 0) return 0;
    return carved_bytes([&](Carver& c) { eq_monitor_carve(c, B, K); });
}
int dccn_eq_monitor_accumulate(const float* chest, const float* chan, int chan_per_symbol, int B, int S, int K,
                               const dccn_metrics* metrics, const float* tx_power, const float* noise_power, float* acc5,
                               float* rms_out, void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    return eq_monitor_accumulate(dccn_eq_monitor{chest, chan, chan_per_symbol, B, S, K, metrics, tx_power, noise_power, acc5, rms_out,
                                                 workspace, workspace_bytes}, (hipStream_t)stream);
}

// ---- the equaliser's pilot bottleneck as one launch per direction (eq_bottleneck.h; eq_step.h eq_bottleneck_*_launch) ----------
int dccn_eq_bottleneck_supported(int B, int SK2, int P) {
    return ((P == 16 || P == 32) && B > 0 && SK2 >= 64 && (SK2 % 64) == 0) ? 1 : 0;
}
size_t dccn_eq_bottleneck_workspace_size(int B, int SK2, int P) {
    if (!dccn_eq_bottleneck_supported(B, SK2, P)) return 0;
    return align_up(eq_bottleneck_part_floats(B, SK2, P) * sizeof(float), 256);
}
int dccn_eq_bottleneck_fwd(const float* y, const float* W1, const float* b1, const float* W2, const float* b2, float* d1,
                           float* d2, int B, int SK2, int P, dccn_stream_t stream) {
    if (!y || !W1 || !W2 || !d1 || !d2 || !eq_bottleneck_ok(B, SK2, P, y, W1, W2) || !aligned16(d1)) return DCCN_ERR_INVALID_ARG;
    return eq_bottleneck_fwd_launch(y, W1, b1, W2, b2, d1, d2, B, SK2, P, (hipStream_t)stream);
}
int dccn_eq_bottleneck_bwd(const float* dd2, const float* d1, const float* y, const float* W1, const float* W2,
                           const float* dy_in, float* dy_out, float* dW1, float* db1, float* dW2, float* db2, int B, int SK2,
                           int P, void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    if (!dd2 || !d1 || !y || !W1 || !W2 || !dy_in || !dy_out || !dW1 || !db1 || !dW2 || !db2 ||
        !eq_bottleneck_ok(B, SK2, P, y, W1, W2) || !aligned16(dd2) || !aligned16(d1))
        return DCCN_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < dccn_eq_bottleneck_workspace_size(B, SK2, P)) return DCCN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const EqBnParts pt = eq_bn_parts(static_cast<float*>(workspace), B, SK2, P);
    DCCN_TRY(eq_bottleneck_bwd_launch(dd2, d1, y, W1, W2, dy_in, dy_out, pt, B, SK2, P, eq_bn_no_riders(), s));
    // (the fused equaliser step leaves these sums to its optimizer launch)
    DCCN_TRY(launch_splitk_reduce2(pt.w2, pt.tiles, (long long)P * SK2, dW2, (long long)P * SK2, pt.b2, (long long)SK2, db2, (long long)SK2, s));
    DCCN_TRY(launch_splitk_reduce2(pt.w1, pt.tiles, (long long)SK2 * P, dW1, (long long)SK2 * P, pt.b1, (long long)P, db1, (long long)P, s));
    return DCCN_OK;
}

}  // extern "C"
