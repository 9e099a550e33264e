// libdccn.so -- per-frame timing alignment from the cyclic prefix (see abi_impl.h for how the library is cut into units)
#include <math.h>

#include "capture_acquire.h"
#include "common.h"
#include "frame_sync.h"
#include "link_group.h"

using namespace dccn;

namespace {
constexpr unsigned kSyncThreads = kSyncWaves * kSyncLanes;

// Every launch of this unit: the kernel's dynamic-LDS limit raised where `lds` needs it, the launch, its check.
template <class Kernel, class Args>
int launch(Kernel kernel, dim3 grid, unsigned threads, size_t lds, dccn_stream_t stream, const Args& args) {
    DCCN_TRY(set_max_dynamic_smem((const void*)kernel, lds));
    hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, (hipStream_t)stream, args);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

// Everything a call decides, before its first launch: a refused call launches nothing.
struct FrameSyncPlan {
    FrameSyncArgs args;
    unsigned blocks;
    size_t lds;
};

int frame_sync_plan(const float* x, int frames, int S, int K, int CP, int W, int out_kin, float* x_out, int32_t* offset,
                    float* metric, FrameSyncPlan* plan) {
    if (!frame_sync_shape_ok(S, K, CP, W) || frames <= 0 || !x || !offset) return DCCN_ERR_INVALID_ARG;
    if (out_kin != K + CP && out_kin != K) return DCCN_ERR_INVALID_ARG;
    if (!aligned16(x) || !aligned16(x_out) || !aligned16(metric)) return DCCN_ERR_INVALID_ARG;
    const int T = S * (K + CP);
    // the cropped rows leave as 16-byte stores too: S * K complex samples per frame, an even count
    if (x_out && out_kin == K && (S * K) % 2 != 0) return DCCN_ERR_INVALID_ARG;
    if (x_out && ranges_overlap(x, (size_t)frames * T * 8, x_out, (size_t)frames * S * out_kin * 8)) return DCCN_ERR_INVALID_ARG;
    plan->args = FrameSyncArgs{x, x_out, offset, metric, frames, S, K, CP, W, out_kin == K ? 1 : 0};
    plan->blocks = (unsigned)ceil_div(frames, kSyncWaves);
    plan->lds = kSyncWaves * frame_sync_lds_per_frame(T);
    return DCCN_OK;
}

// One link of a capture cut.  Where frame 0 starts: `first`, or (first_dev given) what the device holds, which the kernel keeps
// inside [lo, lo + T - 1].
struct CaptureStart {
    long long first;
    const long long* first_dev;     // nullable
    long long lo;
};
struct CaptureSyncPlan {
    CaptureSyncLink link;
    SyncShape shape;
    unsigned blocks;
    size_t lds;
};
// sample_bytes: 8 for a float32 capture; 4 for an sc16 one, whose entries pass the capture's address as `cap` for the checks (the
// capture's extent is n_samples * sample_bytes) and launch kernels that do not read link.cap
int capture_sync_plan(const float* cap, long long n_samples, size_t sample_bytes, CaptureStart at, long long stride, int frames,
                      int S, int K, int CP, int W, int out_kin, float* x_out, int32_t* offset, float* cfo, float* metric,
                      CaptureSyncPlan* plan) {
    if (!capture_sync_shape_ok(S, K, CP, W) || frames <= 0 || !cap || !offset) return DCCN_ERR_INVALID_ARG;
    if (out_kin != K + CP && out_kin != K) return DCCN_ERR_INVALID_ARG;
    if (!aligned16(cap) || !aligned16(x_out) || !aligned16(metric)) return DCCN_ERR_INVALID_ARG;
    const long long T = (long long)S * (K + CP);
    if (x_out && out_kin == K && (S * K) % 2 != 0) return DCCN_ERR_INVALID_ARG;
    if (n_samples <= 0 || n_samples > (1LL << 58) || stride < T) return DCCN_ERR_INVALID_ARG;
    // The start the windows are checked for.  A device start: the LAST one the kernel can clamp to, lo + T - 1 -- every earlier
    // one has its windows inside the capture too, down to lo, whose first window starts at lo - W >= 0.
    long long last = at.first;
    if (at.first_dev) {
        if (!aligned_to<8>(at.first_dev) || at.lo < W || at.lo > n_samples) return DCCN_ERR_INVALID_ARG;
        last = at.lo + T - 1;
    }
    // every window [b_f - W, b_f + T + W) inside the capture, frames not overlapping: last - W >= 0 and
    // last + (frames - 1) stride + T + W <= n_samples, the product taken as a quotient so nothing overflows
    if (last < W || last > n_samples) return DCCN_ERR_INVALID_ARG;
    const long long room = n_samples - last - T - W;
    if (room < 0 || (frames > 1 && stride > room / (frames - 1))) return DCCN_ERR_INVALID_ARG;
    if (x_out && ranges_overlap(cap, (size_t)n_samples * sample_bytes, x_out, (size_t)frames * S * out_kin * 8))
        return DCCN_ERR_INVALID_ARG;
    plan->link = CaptureSyncLink{cap, at.first_dev ? 0 : at.first, stride, at.first_dev, at.first_dev ? at.lo : 0, x_out, offset,
                                 metric, cfo};
    plan->shape = SyncShape{frames, S, K, CP, W, out_kin == K ? 1 : 0};
    plan->blocks = (unsigned)ceil_div(frames, kSyncWaves);
    plan->lds = kSyncWaves * capture_sync_lds_per_frame((int)T, W);
    return DCCN_OK;
}

// The per-frame cut over any of its argument blocks: the frame's own cfo taken out where `cfo` is given.
template <class Args>
int capture_sync_launch(const CaptureSyncPlan& plan, int n_links, bool cfo, const Args& args, dccn_stream_t stream) {
    const dim3 grid(plan.blocks, (unsigned)n_links);
    return cfo ? launch(capture_sync_kernel<SyncFinish::kFrameCfo, Args>, grid, kSyncThreads, plan.lds, stream, args)
               : launch(capture_sync_kernel<SyncFinish::kOffset, Args>, grid, kSyncThreads, plan.lds, stream, args);
}
// the float32 solo cut, from a host start or a device one
int capture_sync_solo_launch(const CaptureSyncPlan& plan, dccn_stream_t stream) {
    return capture_sync_launch(plan, 1, plan.link.cfo != nullptr, CaptureSyncSoloArgs{plan.link, CapOfArgs{}, plan.shape}, stream);
}

// the wide cuts' two device inputs (acquisition's m^ and eps^): given, on 4-byte boundaries
bool wide_inputs_ok(const int32_t* cfo_int_dev, const float* cfo_frac_dev) {
    return cfo_int_dev && cfo_frac_dev && aligned_to<4>(cfo_int_dev) && aligned_to<4>(cfo_frac_dev);
}

// Everything dccn_capture_acquire decides, before its first launch.
struct CaptureAcquirePlan {
    AcqArgs args;
    unsigned sum_blocks;
    size_t lds;
};

int capture_acquire_plan(const float* cap, long long n_samples, long long lo, int J, int S, int K, int CP, const int* pilot_sc,
                         int n_pilot, long long* first_out, float* cfo_out, float* sym_metric, float* phase_metric,
                         void* workspace, size_t workspace_bytes, CaptureAcquirePlan* plan) {
    if (!capture_acquire_shape_ok(S, K, CP, n_pilot, J)) return DCCN_ERR_INVALID_ARG;
    if (!cap || !pilot_sc || !first_out || !cfo_out || !workspace) return DCCN_ERR_INVALID_ARG;
    if (!aligned16(cap) || !aligned16(workspace) || !aligned_to<8>(first_out)) return DCCN_ERR_INVALID_ARG;
    if (!aligned_to<4>(pilot_sc) || !aligned_to<4>(cfo_out) || !aligned_to<4>(sym_metric) || !aligned_to<4>(phase_metric))
        return DCCN_ERR_INVALID_ARG;
    // every read of both stages lies in [lo, lo + (J + 1) T); the documented bound leaves a frame to spare
    const long long T = (long long)S * (K + CP);
    if (lo < 0 || n_samples <= 0 || n_samples > (1LL << 58) || lo > n_samples || (J + 2) * T > n_samples - lo) return DCCN_ERR_INVALID_ARG;
    const AcqWorkspace w = capture_acquire_layout(S, K, CP, J);
    if (workspace_bytes < w.total) return DCCN_ERR_WORKSPACE;
    char* const base = static_cast<char*>(workspace);
    plan->args = AcqArgs{cap, lo, pilot_sc, reinterpret_cast<float4*>(base + w.pe), reinterpret_cast<float*>(base + w.partial),
                         reinterpret_cast<int*>(base + w.rhat), first_out, cfo_out, sym_metric, phase_metric, S, K, CP, J, n_pilot};
    plan->sum_blocks = (unsigned)ceil_div(K + 2 * CP - 1, kAcqSumThreads);
    plan->lds = capture_acquire_lds(S, K, CP, n_pilot);
    return DCCN_OK;
}
// Acquisition's three launches (symbol sums, phase, decision) for n_links links: each kernel with its own argument block.
template <class Sums, class SumsArgs, class Phase, class PhaseArgs, class Decide, class DecideArgs>
int acquire_launch(unsigned sum_blocks, int S, int J, int n_links, size_t phase_lds, unsigned decide_threads, dccn_stream_t stream,
                   Sums sums, const SumsArgs& sums_args, Phase phase, const PhaseArgs& phase_args, Decide decide,
                   const DecideArgs& decide_args) {
    const unsigned G = (unsigned)n_links;
    DCCN_TRY(launch(sums, dim3(sum_blocks, G), kAcqSumThreads, 0, stream, sums_args));
    DCCN_TRY(launch(phase, dim3((unsigned)S, (unsigned)J, G), kAcqThreads, phase_lds, stream, phase_args));
    return launch(decide, dim3(G), decide_threads, 0, stream, decide_args);
}

// ---- the grouped entries: every link through the solo plan above, then what only a group can get wrong (link_group.h) ------------
struct FrameSyncGroupPlan {
    FrameSyncGroupArgs args;
    unsigned blocks;
    size_t lds;
};
int frame_sync_group_plan(int n_links, const dccn_frame_link* links, int frames, int S, int K, int CP, int W, int out_kin,
                          FrameSyncGroupPlan* plan) {
    plan->args = FrameSyncGroupArgs{};
    return group_plan(n_links, links, [&](int i, const dccn_frame_link& l, LinkRanges* r) -> int {
        FrameSyncPlan one;
        DCCN_TRY(frame_sync_plan(l.x, frames, S, K, CP, W, out_kin, l.x_out, l.offset, l.metric, &one));
        if (!aligned_to<4>(l.cfo)) return DCCN_ERR_INVALID_ARG;
        const FrameSyncArgs& a = one.args;
        plan->args.link[i] = FrameSyncLink{a.x, a.x_out, a.offset, a.metric, l.cfo};
        plan->args.frames = a.frames; plan->args.S = a.S; plan->args.K = a.K; plan->args.CP = a.CP; plan->args.W = a.W;
        plan->args.crop = a.crop;
        plan->blocks = one.blocks;
        plan->lds = one.lds;
        r->out(l.x_out, (size_t)frames * S * out_kin * 8);
        r->out(l.offset, (size_t)frames * 4);
        r->out(l.cfo, (size_t)frames * 4);
        r->out(l.metric, (size_t)frames * (2 * W + 1) * 4);
        r->in(l.x, (size_t)frames * S * (K + CP) * 8);
        return DCCN_OK;
    }, &dccn_frame_link::x_out, &dccn_frame_link::cfo, &dccn_frame_link::metric);
}

struct CaptureSyncGroupPlan {
    CaptureSyncGroupArgs args;
    CaptureSyncPlan one;        // the shape and the geometry: any link's
};
int capture_sync_group_plan(int n_links, const dccn_capture_link* links, int frames, int S, int K, int CP, int W, int out_kin,
                            CaptureSyncGroupPlan* plan) {
    plan->args = CaptureSyncGroupArgs{};
    return group_plan(n_links, links, [&](int i, const dccn_capture_link& l, LinkRanges* r) -> int {
        DCCN_TRY(capture_sync_plan(l.cap, l.n_samples, 8, CaptureStart{l.first, l.first_dev, l.lo}, l.stride, frames, S, K, CP, W,
                                   out_kin, l.x_out, l.offset, l.cfo, l.metric, &plan->one));
        if (!aligned_to<4>(l.cfo)) return DCCN_ERR_INVALID_ARG;
        plan->args.link[i] = plan->one.link;
        plan->args.shape = plan->one.shape;
        r->out(l.x_out, (size_t)frames * S * out_kin * 8);
        r->out(l.offset, (size_t)frames * 4);
        r->out(l.cfo, (size_t)frames * 4);
        r->out(l.metric, (size_t)frames * (2 * W + 1) * 4);
        r->in(l.cap, (size_t)l.n_samples * 8);
        r->in(l.first_dev, 8);
        return DCCN_OK;
    }, &dccn_capture_link::x_out, &dccn_capture_link::cfo, &dccn_capture_link::metric);
}

// dccn_capture_sync_pooled(_grouped): every link through the per-frame entry's own plan (so the windows, the alignment and the
// cap / x_out overlap are judged by the same code), then what the pooled call adds.
size_t pooled_workspace_bytes(int frames) { return frames > 0 ? ((size_t)frames * sizeof(float2) + 15) & ~(size_t)15 : 0; }

struct PooledGroupPlan {
    PooledGroupArgs args;
    unsigned blocks;
    size_t lds_estimate, lds_cut;
};
int pooled_group_plan(int n_links, const dccn_pooled_link* links, int frames, int S, int K, int CP, int W, int out_kin,
                      PooledGroupPlan* plan, size_t sample_bytes = 8) {
    plan->args = PooledGroupArgs{};
    DCCN_TRY(group_plan(n_links, links, [&](int i, const dccn_pooled_link& l, LinkRanges* r) -> int {
        CaptureSyncPlan one;
        DCCN_TRY(capture_sync_plan(l.cap, l.n_samples, sample_bytes, CaptureStart{l.first, l.first_dev, l.lo}, l.stride, frames, S, K,
                                   CP, W, out_kin, l.x_out, l.offset, l.cfo, l.metric, &one));
        if (!l.x_out || !l.cfo || !aligned_to<4>(l.cfo)) return DCCN_ERR_INVALID_ARG;
        if (!l.workspace || !aligned16(l.workspace)) return DCCN_ERR_INVALID_ARG;
        plan->args.link[i] = PooledLink{one.link, static_cast<float2*>(l.workspace)};
        plan->args.shape = one.shape;
        plan->blocks = one.blocks;
        plan->lds_estimate = one.lds;
        plan->lds_cut = kSyncWaves * capture_cut_lds_per_frame(S * (K + CP));
        r->out(l.x_out, (size_t)frames * S * out_kin * 8);
        r->out(l.offset, (size_t)frames * 4);
        r->out(l.cfo, 4);
        r->out(l.metric, (size_t)frames * (2 * W + 1) * 4);
        r->out(l.workspace, pooled_workspace_bytes(frames));
        r->in(l.cap, (size_t)l.n_samples * sample_bytes);
        r->in(l.first_dev, 8);
        return DCCN_OK;
    }, &dccn_pooled_link::metric));
    for (int i = 0; i < n_links; ++i)
        if (links[i].workspace_bytes < pooled_workspace_bytes(frames)) return DCCN_ERR_WORKSPACE;
    return DCCN_OK;
}
// The pooled call's three launches: the estimate and the cut with their argument blocks, the sum between them over the plan's own
// table (it reads no capture).
template <class Estimate, class EstimateArgs, class Cut, class CutArgs>
int pooled_launch(const PooledGroupPlan& plan, int n_links, dccn_stream_t stream, Estimate estimate, const EstimateArgs& estimate_args,
                  Cut cut, const CutArgs& cut_args) {
    const dim3 grid(plan.blocks, (unsigned)n_links);
    DCCN_TRY(launch(estimate, grid, kSyncThreads, plan.lds_estimate, stream, estimate_args));
    DCCN_TRY(launch(capture_pool_reduce_kernel, dim3((unsigned)n_links), kSyncLanes, 0, stream, plan.args));
    return launch(cut, grid, kSyncThreads, plan.lds_cut, stream, cut_args);
}

struct CaptureAcquireGroupPlan {
    AcqGroupArgs args;
    unsigned sum_blocks;
    size_t lds;
};
int capture_acquire_group_plan(int n_links, const dccn_acquire_link* links, int J, int S, int K, int CP, int n_pilot,
                               CaptureAcquireGroupPlan* plan) {
    plan->args = AcqGroupArgs{};
    return group_plan(n_links, links, [&](int i, const dccn_acquire_link& l, LinkRanges* r) -> int {
        CaptureAcquirePlan one;
        DCCN_TRY(capture_acquire_plan(l.cap, l.n_samples, l.lo, J, S, K, CP, l.pilot_sc, n_pilot, l.first_out, l.cfo_out, l.sym_metric,
                                      l.phase_metric, l.workspace, l.workspace_bytes, &one));
        const AcqArgs& a = one.args;
        plan->args.link[i] = AcqLink{a.cap, a.lo, a.pilot_sc, a.pe, a.partial, a.rhat, a.first_out, a.cfo_out, a.sym_metric,
                                     a.phase_metric};
        plan->args.S = S; plan->args.K = K; plan->args.CP = CP; plan->args.J = J; plan->args.n_pilot = n_pilot;
        plan->sum_blocks = one.sum_blocks;
        plan->lds = one.lds;
        r->out(l.first_out, 8);
        r->out(l.cfo_out, 4);
        r->out(l.sym_metric, (size_t)(K + CP) * 4);
        r->out(l.phase_metric, (size_t)S * 4);
        r->out(l.workspace, capture_acquire_layout(S, K, CP, J).total);
        r->in(l.cap, (size_t)l.n_samples * 8);
        r->in(l.pilot_sc, (size_t)n_pilot * 4);
        return DCCN_OK;
    }, &dccn_acquire_link::sym_metric, &dccn_acquire_link::phase_metric);
}

// ---- 16-bit integer I/Q captures: the float32 plans with the capture's extent taken as 4 bytes per sample -----------------------
bool sc16_scale_ok(float scale) { return isfinite(scale) && scale > 0.f; }
const float* sc16_as_checked(const int16_t* cap) { return reinterpret_cast<const float*>(cap); }    // (an address to check, never read)
}  // namespace

extern "C" {

int dccn_frame_sync_supported(int S, int K, int CP, int W) { return frame_sync_shape_ok(S, K, CP, W) ? 1 : 0; }

int dccn_frame_sync(const float* x, int frames, int S, int K, int CP, int W, int out_kin, float* x_out, int32_t* offset,
                    float* metric, dccn_stream_t stream) {
    FrameSyncPlan plan;
    DCCN_TRY(frame_sync_plan(x, frames, S, K, CP, W, out_kin, x_out, offset, metric, &plan));
    return launch(frame_sync_kernel, dim3(plan.blocks), kSyncThreads, plan.lds, stream, plan.args);
}

int dccn_frame_sync_cfo(const float* x, int frames, int S, int K, int CP, int W, int out_kin, float* x_out, int32_t* offset,
                        float* cfo, float* metric, dccn_stream_t stream) {
    FrameSyncPlan plan;
    DCCN_TRY(frame_sync_plan(x, frames, S, K, CP, W, out_kin, x_out, offset, metric, &plan));
    if (!cfo) return DCCN_ERR_INVALID_ARG;
    DCCN_NO_CHAINS();                         // (the launch carries no chain table: inside a group it would serve chain 0 only)
    return launch(frame_sync_cfo_kernel, dim3(plan.blocks), kSyncThreads, plan.lds, stream, FrameSyncCfoArgs{plan.args, cfo});
}

int dccn_capture_sync_supported(int S, int K, int CP, int W) { return capture_sync_shape_ok(S, K, CP, W) ? 1 : 0; }

int dccn_capture_sync(const float* cap, long long n_samples, long long first, long long stride, int frames, int S, int K, int CP,
                      int W, int out_kin, float* x_out, int32_t* offset, float* cfo, float* metric, dccn_stream_t stream) {
    CaptureSyncPlan plan;
    DCCN_TRY(capture_sync_plan(cap, n_samples, 8, CaptureStart{first, nullptr, 0}, stride, frames, S, K, CP, W, out_kin, x_out, offset,
                               cfo, metric, &plan));
    DCCN_NO_CHAINS();
    return capture_sync_solo_launch(plan, stream);
}

int dccn_capture_sync_at(const float* cap, long long n_samples, const long long* first_dev, long long lo, long long stride,
                         int frames, int S, int K, int CP, int W, int out_kin, float* x_out, int32_t* offset, float* cfo,
                         float* metric, dccn_stream_t stream) {
    if (!first_dev) return DCCN_ERR_INVALID_ARG;
    CaptureSyncPlan plan;
    DCCN_TRY(capture_sync_plan(cap, n_samples, 8, CaptureStart{0, first_dev, lo}, stride, frames, S, K, CP, W, out_kin, x_out, offset,
                               cfo, metric, &plan));
    DCCN_NO_CHAINS();
    return capture_sync_solo_launch(plan, stream);
}

int dccn_capture_acquire_supported(int S, int K, int CP, int n_pilot, int J) {
    return capture_acquire_shape_ok(S, K, CP, n_pilot, J) ? 1 : 0;
}

size_t dccn_capture_acquire_workspace_size(int S, int K, int CP, int n_pilot, int J) {
    return capture_acquire_shape_ok(S, K, CP, n_pilot, J) ? capture_acquire_layout(S, K, CP, J).total : 0;
}

int dccn_capture_acquire(const float* cap, long long n_samples, long long lo, int J, int S, int K, int CP, const int* pilot_sc,
                         int n_pilot, long long* first_out, float* cfo_out, float* sym_metric, float* phase_metric,
                         void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    CaptureAcquirePlan plan;
    DCCN_TRY(capture_acquire_plan(cap, n_samples, lo, J, S, K, CP, pilot_sc, n_pilot, first_out, cfo_out, sym_metric, phase_metric,
                                  workspace, workspace_bytes, &plan));
    DCCN_NO_CHAINS();
    return acquire_launch(plan.sum_blocks, S, J, 1, plan.lds, kAcqMaxS, stream, acq_symbol_sums_kernel, plan.args, acq_phase_kernel,
                          plan.args, acq_decide_kernel, plan.args);
}

// ---- several links per launch: the link table is the call's own, so inside a ChainScope these refuse like the solo entries ----
int dccn_frame_sync_grouped(int n_links, const dccn_frame_link* links, int frames, int S, int K, int CP, int W, int out_kin,
                            dccn_stream_t stream) {
    FrameSyncGroupPlan plan;
    DCCN_TRY(frame_sync_group_plan(n_links, links, frames, S, K, CP, W, out_kin, &plan));
    DCCN_NO_CHAINS();
    const dim3 grid(plan.blocks, (unsigned)n_links);
    return links[0].cfo ? launch(frame_sync_grouped_kernel<true>, grid, kSyncThreads, plan.lds, stream, plan.args)
                        : launch(frame_sync_grouped_kernel<false>, grid, kSyncThreads, plan.lds, stream, plan.args);
}

int dccn_capture_sync_grouped(int n_links, const dccn_capture_link* links, int frames, int S, int K, int CP, int W, int out_kin,
                              dccn_stream_t stream) {
    CaptureSyncGroupPlan plan;
    DCCN_TRY(capture_sync_group_plan(n_links, links, frames, S, K, CP, W, out_kin, &plan));
    DCCN_NO_CHAINS();
    return capture_sync_launch(plan.one, n_links, links[0].cfo != nullptr, plan.args, stream);
}

int dccn_capture_acquire_grouped(int n_links, const dccn_acquire_link* links, int J, int S, int K, int CP, int n_pilot,
                                 dccn_stream_t stream) {
    CaptureAcquireGroupPlan plan;
    DCCN_TRY(capture_acquire_group_plan(n_links, links, J, S, K, CP, n_pilot, &plan));
    DCCN_NO_CHAINS();
    return acquire_launch(plan.sum_blocks, S, J, n_links, plan.lds, kAcqMaxS, stream, acq_symbol_sums_grouped_kernel, plan.args,
                          acq_phase_grouped_kernel, plan.args, acq_decide_grouped_kernel, plan.args);
}

// ---- one carrier offset per capture: the solo entry is the grouped one with one link -----------------------------------------
size_t dccn_capture_sync_pooled_workspace_size(int frames) { return pooled_workspace_bytes(frames); }

int dccn_capture_sync_pooled_grouped(int n_links, const dccn_pooled_link* links, int frames, int S, int K, int CP, int W,
                                     int out_kin, dccn_stream_t stream) {
    PooledGroupPlan plan;
    DCCN_TRY(pooled_group_plan(n_links, links, frames, S, K, CP, W, out_kin, &plan));
    DCCN_NO_CHAINS();
    return pooled_launch(plan, n_links, stream, capture_pool_estimate_kernel<PooledGroupArgs>, plan.args,
                         capture_pool_cut_kernel<false, PooledGroupArgs>, plan.args);
}

int dccn_capture_sync_pooled(const float* cap, long long n_samples, long long first, const long long* first_dev, long long lo,
                             long long stride, int frames, int S, int K, int CP, int W, int out_kin, float* x_out, int32_t* offset,
                             float* cfo_out, float* metric, void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    const dccn_pooled_link link{cap, n_samples, first, first_dev, lo, stride, x_out, offset, cfo_out, metric, workspace, workspace_bytes};
    return dccn_capture_sync_pooled_grouped(1, &link, frames, S, K, CP, W, out_kin, stream);
}

// ---- 16-bit integer I/Q captures, converted inside the launches ----------------------------------------------------------------
int dccn_capture_sync_sc16(const int16_t* cap, long long n_samples, float scale, long long first, const long long* first_dev,
                           long long lo, long long stride, int frames, int S, int K, int CP, int W, int out_kin, float* x_out,
                           int32_t* offset, float* cfo, float* metric, dccn_stream_t stream) {
    if (!sc16_scale_ok(scale)) return DCCN_ERR_INVALID_ARG;
    CaptureSyncPlan plan;
    DCCN_TRY(capture_sync_plan(sc16_as_checked(cap), n_samples, 4, CaptureStart{first, first_dev, lo}, stride, frames, S, K, CP, W,
                               out_kin, x_out, offset, cfo, metric, &plan));
    DCCN_NO_CHAINS();
    plan.link.cap = nullptr;
    return capture_sync_launch(plan, 1, cfo != nullptr, CaptureSyncSc16Args{plan.link, CapSc16{cap, scale}, plan.shape}, stream);
}

int dccn_capture_sync_pooled_sc16(const int16_t* cap, long long n_samples, float scale, long long first, const long long* first_dev,
                                  long long lo, long long stride, int frames, int S, int K, int CP, int W, int out_kin, float* x_out,
                                  int32_t* offset, float* cfo_out, float* metric, void* workspace, size_t workspace_bytes,
                                  dccn_stream_t stream) {
    if (!sc16_scale_ok(scale)) return DCCN_ERR_INVALID_ARG;
    // the pooled call's plan for one link; the link struct keeps its layout, its `cap` carries the address for the checks
    const dccn_pooled_link link{sc16_as_checked(cap), n_samples, first, first_dev, lo, stride, x_out, offset, cfo_out, metric, workspace,
                                workspace_bytes};
    PooledGroupPlan plan;
    DCCN_TRY(pooled_group_plan(1, &link, frames, S, K, CP, W, out_kin, &plan, 4));
    DCCN_NO_CHAINS();
    plan.args.link[0].s.cap = nullptr;
    const PooledSc16Args args{plan.args.link[0], CapSc16{cap, scale}, plan.args.shape};
    return pooled_launch(plan, 1, stream, capture_pool_estimate_kernel<PooledSc16Args>, args,
                         capture_pool_cut_kernel<false, PooledSc16Args>, args);
}

int dccn_capture_acquire_sc16(const int16_t* cap, long long n_samples, float scale, long long lo, int J, int S, int K, int CP,
                              const int* pilot_sc, int n_pilot, long long* first_out, float* cfo_out, float* sym_metric,
                              float* phase_metric, void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    if (!sc16_scale_ok(scale)) return DCCN_ERR_INVALID_ARG;
    CaptureAcquirePlan plan;        // (the plan looks at sample counts and the base's alignment: nothing depends on the sample's size)
    DCCN_TRY(capture_acquire_plan(sc16_as_checked(cap), n_samples, lo, J, S, K, CP, pilot_sc, n_pilot, first_out, cfo_out, sym_metric,
                                  phase_metric, workspace, workspace_bytes, &plan));
    DCCN_NO_CHAINS();
    plan.args.cap = nullptr;
    const AcqSc16Args args{plan.args, CapSc16{cap, scale}};
    return acquire_launch(plan.sum_blocks, S, J, 1, plan.lds, kAcqMaxS, stream, acq_symbol_sums_sc16_kernel, args, acq_phase_sc16_kernel,
                          args, acq_decide_kernel, plan.args);
}

// ---- carrier offsets beyond half a subcarrier spacing: acquisition over (q, m), the cut with the whole offset taken out ---------
int dccn_capture_acquire_wide_supported(int S, int K, int CP, int n_pilot, int J, int M) {
    return capture_acquire_wide_shape_ok(S, K, CP, n_pilot, J, M) ? 1 : 0;
}

size_t dccn_capture_acquire_wide_workspace_size(int S, int K, int CP, int n_pilot, int J, int M) {
    return capture_acquire_wide_shape_ok(S, K, CP, n_pilot, J, M) ? capture_acquire_wide_layout(S, K, CP, J, M).total : 0;
}

int dccn_capture_acquire_wide(const float* cap, long long n_samples, long long lo, int J, int S, int K, int CP, const int* pilot_sc,
                              int n_pilot, int M, long long* first_out, float* cfo_out, int32_t* cfo_int_out, float* sym_metric,
                              float* phase_metric, void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    if (!capture_acquire_wide_shape_ok(S, K, CP, n_pilot, J, M)) return DCCN_ERR_INVALID_ARG;
    if (!cfo_int_out || !aligned_to<4>(cfo_int_out)) return DCCN_ERR_INVALID_ARG;
    const AcqWorkspace w = capture_acquire_wide_layout(S, K, CP, J, M);
    // the narrow call's checks (the samples read are the same); its workspace is the M = 0 layout, a prefix of this one
    CaptureAcquirePlan plan;
    DCCN_TRY(capture_acquire_plan(cap, n_samples, lo, J, S, K, CP, pilot_sc, n_pilot, first_out, cfo_out, sym_metric, phase_metric,
                                  workspace, workspace_bytes, &plan));
    if (workspace_bytes < w.total) return DCCN_ERR_WORKSPACE;
    DCCN_NO_CHAINS();
    AcqWideArgs args{plan.args, cfo_int_out, M};
    args.a.rhat = reinterpret_cast<int*>(static_cast<char*>(workspace) + w.rhat);
    return acquire_launch(plan.sum_blocks, S, J, 1, capture_acquire_wide_lds(S, K, CP, n_pilot, M), kAcqWideThreads, stream,
                          acq_symbol_sums_kernel, args.a, acq_phase_wide_kernel, args, acq_decide_wide_kernel, args);
}

int dccn_capture_sync_wide(const float* cap, long long n_samples, const long long* first_dev, long long lo, long long stride,
                           int frames, int S, int K, int CP, int W, int out_kin, float* x_out, int32_t* offset, float* cfo,
                           float* metric, const int32_t* cfo_int_dev, const float* cfo_frac_dev, dccn_stream_t stream) {
    if (!first_dev) return DCCN_ERR_INVALID_ARG;
    CaptureSyncPlan plan;
    DCCN_TRY(capture_sync_plan(cap, n_samples, 8, CaptureStart{0, first_dev, lo}, stride, frames, S, K, CP, W, out_kin, x_out, offset,
                               cfo, metric, &plan));
    if (!cfo || !wide_inputs_ok(cfo_int_dev, cfo_frac_dev)) return DCCN_ERR_INVALID_ARG;
    DCCN_NO_CHAINS();
    return launch(capture_sync_kernel<SyncFinish::kWide, CaptureSyncWideArgs>, dim3(plan.blocks), kSyncThreads, plan.lds, stream,
                  CaptureSyncWideArgs{{plan.link, CapOfArgs{}, plan.shape}, CfoWide{cfo_int_dev, cfo_frac_dev}});
}

size_t dccn_capture_sync_pooled_wide_workspace_size(int frames) { return frames > 0 ? pooled_workspace_bytes(frames) + 16 : 0; }

int dccn_capture_sync_pooled_wide(const float* cap, long long n_samples, long long first, const long long* first_dev, long long lo,
                                  long long stride, int frames, int S, int K, int CP, int W, int out_kin, float* x_out,
                                  int32_t* offset, float* cfo_out, float* metric, const int32_t* cfo_int_dev,
                                  const float* cfo_frac_dev, void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    // the pooled call's plan with the fraction's slot (behind Gamma_f in the workspace) where it has cfo_out
    const size_t gamma_bytes = pooled_workspace_bytes(frames);
    const dccn_pooled_link link{cap, n_samples, first, first_dev, lo, stride, x_out, offset, cfo_out, metric, workspace, workspace_bytes};
    PooledGroupPlan plan;
    DCCN_TRY(pooled_group_plan(1, &link, frames, S, K, CP, W, out_kin, &plan));
    if (!wide_inputs_ok(cfo_int_dev, cfo_frac_dev)) return DCCN_ERR_INVALID_ARG;
    if (workspace_bytes < gamma_bytes + 16) return DCCN_ERR_WORKSPACE;
    DCCN_NO_CHAINS();
    plan.args.link[0].s.cfo = reinterpret_cast<float*>(static_cast<char*>(workspace) + gamma_bytes);
    return pooled_launch(plan, 1, stream, capture_pool_estimate_kernel<PooledGroupArgs>, plan.args,
                         capture_pool_cut_kernel<true, PooledWideArgs>,
                         PooledWideArgs{{plan.args.link[0], CapOfArgs{}, plan.args.shape}, CfoWide{cfo_int_dev, cfo_frac_dev}, cfo_out});
}

}  // extern "C"
