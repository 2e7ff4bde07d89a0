// The batched front end's lifecycle: create (switches, sizes, frames, the
// device / pinned / host-coherent blocks, the pool, streams and events),
// destroy, the resident and streamed frame ring, init.
#include <algorithm>
#include <cctype>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <thread>

#include "frontend_state.hpp"

namespace svo {

FeSwitches fe_read_switches(const svo_frontend_config& c) {
    auto env = [](const char* name) { return std::getenv(name); };
    auto is = [&](const char* name, char v) {
        const char* e = env(name);
        return e && e[0] == v;
    };
    FeSwitches sw;
    sw.fast_pre = is("SVO_FE_FAST_PRE", '0') ? 0 : 1;
    sw.pre_after_post = is("SVO_FE_PRE_AFTER_POST", '0') ? 0 : 1;
    sw.spec_margin = env("SVO_FE_SPEC_MARGIN") ? std::atoi(env("SVO_FE_SPEC_MARGIN")) : 32;
    sw.spec_early = is("SVO_FE_SPEC_EARLY", '0') ? 0 : 1;
    sw.trace = is("SVO_FE_TRACE", '1');
    sw.device_fits = is("SVO_FE_DEVICE_FITS", '1');
    sw.debug = is("SVO_FE_DEBUG", '1');
    sw.pool_pin = env("SVO_POOL_PIN") ? (is("SVO_POOL_PIN", '1') ? 1 : 0) : -1;
    sw.pool_spin_us = pool_spin_env();
    // the deferred keyframe: SVO_FE_DEFER_KF=1 / 0, or by default where the batch is
    // large enough (kDeferMinFeatures) unless a switch of the speculative schedule is
    // set (they keep meaning what they meant); it speculates nothing
    if (c.keyframe_rule == SVO_KF_EVERY && !c.use_orb)
        sw.defer_kf = env("SVO_FE_DEFER_KF")
                          ? is("SVO_FE_DEFER_KF", '1')
                          : !env("SVO_FE_SPEC_MARGIN") && !env("SVO_FE_SPEC_EARLY") &&
                                (long long)c.n_seq * c.n_features >= kDeferMinFeatures;
    if (sw.defer_kf) {
        sw.spec_margin = -1;
        sw.spec_early = 0;
    }
    if (c.use_orb) {  // ORB: detection at the keyframe, the serial keyframe path
        sw.fast_pre = 0;
        sw.spec_margin = -1;
        sw.spec_early = 0;
    }
    return sw;
}

}  // namespace svo

using namespace svo;

namespace {

// LOCAL_RANK / LOCAL_WORLD_SIZE as torch.distributed.run sets them (one process per GPU)
int local_rank_env() {
    const char* e = std::getenv("LOCAL_RANK");
    return e ? std::max(0, std::atoi(e)) : 0;
}
int local_world_env() {
    const char* e = std::getenv("LOCAL_WORLD_SIZE");
    return e ? std::max(1, std::atoi(e)) : 1;
}

// NUMA node of HIP device d (-1: unknown), from its PCI address in sysfs
int device_numa_node(int d) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof(bus), d) != hipSuccess) return -1;
    std::string id(bus);
    for (auto& ch : id) ch = (char)std::tolower((unsigned char)ch);
    std::ifstream f("/sys/bus/pci/devices/" + id + "/numa_node");
    int v = -1;
    if (f) f >> v;
    return v;
}

hipError_t fe_make_stream(hipStream_t* st, int priority) {
    return hipStreamCreateWithPriority(st, hipStreamNonBlocking, priority);
}

// ---- svo_frontend_create's parts, in its order ----

void create_sizes(svo_frontend* fe) {
    const svo_frontend_config& c = fe->cfg;
    fe->S = c.n_seq;
    fe->T = c.n_frames;
    fe->W = c.width;
    fe->H = c.height;
    fe->CAP = (c.n_features + 63) & ~63;
    fe->WORDS = (fe->CAP + 31) / 32;
    fe->KCAP = std::max(4 * fe->CAP, 8192);
    fe->BCAP = ((c.bucket_size > 0) ? (c.height / c.bucket_size + 1) * (c.width / c.bucket_size + 1) * c.per_bucket
                                    : 1) + 64;
    fe->MAPCAP = fe->CAP * (c.n_frames + 2);
    fe->npx = (size_t)c.width * c.height;
    fe->ml = lk_levels_for_window(c.width, c.height, c.win, c.win, c.max_level);
    fe->ml_st = lk_levels_for_window(c.width, c.height, c.stereo_win, c.stereo_win, c.stereo_max_level);
    fe->nlev = std::max(fe->ml, fe->ml_st) + 1;
    fe->bscr = c.bucket_size > 0 ? bucket_scratch_ints(c.width, c.height, c.bucket_size, c.per_bucket, fe->KCAP) : 1;
}

// frames: left and right pyramids of every resident stereo pair
int create_frames(svo_frontend* fe) {
    const svo_frontend_config& c = fe->cfg;
    const int S = fe->S;
    fe->frames.assign((size_t)S * fe->T, nullptr);
    fe->frames_r.assign((size_t)S * fe->T, nullptr);
    for (auto* v : {&fe->frames, &fe->frames_r})
        for (auto& f : *v) {
            int rc = svo_image_create(fe->ctx, c.width, c.height, fe->nlev - 1, &f);
            if (rc) return rc;
        }
    fe->desc_host.resize((size_t)fe->T * S);
    fe->desc_r_host.resize((size_t)fe->T * S);
    for (int t = 0; t < fe->T; t++)
        for (int s = 0; s < S; s++) {
            fe->desc_host[(size_t)t * S + s] = fe->frames[(size_t)s * fe->T + t]->desc;
            fe->desc_r_host[(size_t)t * S + s] = fe->frames_r[(size_t)s * fe->T + t]->desc;
        }
    return SVO_OK;
}

// device state: one allocation, laid out by the sequence below
int create_device_state(svo_frontend* fe) {
    svo_ctx* ctx = fe->ctx;
    const svo_frontend_config& c = fe->cfg;
    const int S = fe->S, CAP = fe->CAP;
    auto layout = [&](Carver& p) {
        fe->d_desc = p.take<PyrDesc>((size_t)fe->T * S);
        fe->d_desc_r = p.take<PyrDesc>((size_t)fe->T * S);
        fe->xyA = p.take<float>(2 * (size_t)S * CAP);
        fe->next_xy = p.take<float>(2 * (size_t)S * CAP);
        fe->st_xy = p.take<float>(2 * (size_t)S * CAP);
        fe->st_next = p.take<float>(2 * (size_t)S * CAP);
        fe->st_status = p.take<uint8_t>((size_t)S * CAP);
        fe->st_X = p.take<float4>((size_t)S * CAP);
        fe->st_n = p.take<int>(S);
        fe->pend0 = p.take<int>(S);
        fe->pend_n = p.take<int>(S);
        fe->spec_n = p.take<int>(S);
        fe->n_main = p.take<int>(S);
        fe->kps = p.take<float>(3 * (size_t)S * fe->KCAP);
        fe->cand = p.take<float>(2 * (size_t)S * fe->BCAP);
        fe->midA = p.take<int>((size_t)S * CAP);
        fe->midB = p.take<int>((size_t)S * CAP);
        fe->iters = p.take<int>((size_t)S * CAP);
        fe->nA = p.take<int>(S);
        fe->kn = p.take<int>(S);
        fe->bn = p.take<int>(S);
        fe->map_n = p.take<int>(S);
        fe->added = p.take<int>(S);
        fe->rowcnt = p.take<int>((size_t)S * c.height);
        fe->scr = p.take<int>(fe->bscr * S);
        fe->status = p.take<uint8_t>((size_t)S * CAP);
        fe->fbits = p.take<unsigned long long>((size_t)S * c.height * ((c.width + 63) / 64));
        fe->rowoff = p.take<int>((size_t)S * c.height);
        fe->map = p.take<double>(3 * (size_t)S * fe->MAPCAP);
        fe->box_binned = p.take<float>(2 * (size_t)S * CAP);
        fe->box_band = p.take<int>((size_t)S * fast_box_cells(c.width, c.height));
        for (int k = 0; k < 2; k++) {
            fe->xyB_b[k] = p.take<float>(2 * (size_t)S * CAP);
            fe->obj_b[k] = p.take<float>(3 * (size_t)S * CAP);
            fe->nB_b[k] = p.take<int>(S);
        }
        fe->xyB = fe->xyB_b[0];
        fe->obj = fe->obj_b[0];
        fe->nB = fe->nB_b[0];
    };
    const size_t bytes = layout_bytes(layout);
    if (hipMalloc(&fe->dmem, bytes) != hipSuccess)
        return set_error(ctx, SVO_ERR_HIP, "svo_frontend_create: hipMalloc(%zu)", bytes);
    layout_place(fe->dmem, layout);
    (void)hipMemsetAsync(fe->dmem, 0, bytes, ctx->stream);
    return SVO_OK;
}

// host mirrors (pinned): both parities of the full point copies
int create_pinned_mirrors(svo_frontend* fe) {
    const int S = fe->S, CAP = fe->CAP;
    auto layout = [&](Carver& p) {
        for (int k = 0; k < 2; k++) {
            fe->h_xyB_b[k] = p.take<float>(2 * (size_t)S * CAP);
            fe->h_obj_b[k] = p.take<float>(3 * (size_t)S * CAP);
        }
    };
    if (hipHostMalloc(&fe->hmem, layout_bytes(layout), hipHostMallocDefault) != hipSuccess)
        return set_error(fe->ctx, SVO_ERR_HIP, "svo_frontend_create: hipHostMalloc");
    layout_place(fe->hmem, layout);
    fe->h_xyB = fe->h_xyB_b[0];
    fe->h_obj = fe->h_obj_b[0];
    return SVO_OK;
}

int create_coherent(svo_frontend* fe) {
    svo_ctx* ctx = fe->ctx;
    const int S = fe->S;
    // zero-copy scoring buffers (coherent: the kernel's writes are visible to the
    // host once the stream is synchronised)
    {
        auto layout = [&](Carver& p) {
            fe->z_hyps = p.take<double>(12 * (size_t)S * kRansacChunk);
            fe->z_bits = p.take<uint32_t>((size_t)S * kRansacChunk * fe->WORDS);
            fe->z_cnt = p.take<int>((size_t)S * kRansacChunk);
        };
        if (hipHostMalloc(&fe->zmem, layout_bytes(layout), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) {
            fe->zmem = nullptr;
            return set_error(ctx, SVO_ERR_HIP, "svo_frontend_create: host-coherent scoring buffers");
        }
        layout_place(fe->zmem, layout);
    }
    // host-coherent outputs the kernels write directly (no D2H copies on the
    // critical path): post-LK counts / iteration sums / RANSAC subsets, the
    // keyframe's counts; the inlier bits the tail and the statistics read (parity
    // pair); the keyframe targets the keyframe kernels read
    {
        auto layout = [&](Carver& p) {
            fe->h_nB = p.take<int>(S);
            fe->h_nA = p.take<int>(S);
            fe->h_added = p.take<int>(S);
            fe->h_target = p.take<int>(S);
            fe->h_over = p.take<int>(S);
            fe->h_itsum = p.take<long long>(S);
            fe->h_samp = p.take<float>((size_t)kSampleFloats * kRansacPrefetch * S);
            fe->h_best_b[0] = p.take<uint32_t>((size_t)S * fe->WORDS);
            fe->h_best_b[1] = p.take<uint32_t>((size_t)S * fe->WORDS);
            fe->h_stats = p.take<double>(kSqpnpStats * (size_t)S);
            fe->h_pose = p.take<double>(12 * (size_t)S);
            fe->h_pose6 = p.take<double>(6 * (size_t)S);
            fe->h_fitin = p.take<SqpnpFitIn>((size_t)S);
        };
        const size_t zb = layout_bytes(layout);
        if (hipHostMalloc(&fe->zout, zb, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) {
            fe->zout = nullptr;
            return set_error(ctx, SVO_ERR_HIP, "svo_frontend_create: host-coherent alloc");
        }
        std::memset(fe->zout, 0, zb);
        layout_place(fe->zout, layout);
        fe->h_best = fe->h_best_b[0];
        for (int s = 0; s < S; s++) fe_set_pose(fe, s, false, nullptr, nullptr);
    }
    return SVO_OK;
}

// derivative pyramids of three frames of every sequence (t - 1: LK's prev,
// t, and t + 1, built beside LK(t))
int create_deriv_pyramids(svo_frontend* fe) {
    svo_ctx* ctx = fe->ctx;
    const svo_frontend_config& c = fe->cfg;
    const int S = fe->S;
    size_t doff[kMaxLevels];
    int dpitch[kMaxLevels];
    const size_t dbytes = (deriv_layout(c.width, c.height, fe->nlev, doff, dpitch) + 255) & ~(size_t)255;
    char* base;
    auto layout = [&](Carver& p) {
        fe->d_der = p.take<DerivDesc>(3 * (size_t)S);
        base = p.take<char>(dbytes * 3 * S);
    };
    if (hipMalloc(&fe->dermem, layout_bytes(layout)) != hipSuccess)
        return set_error(ctx, SVO_ERR_HIP, "svo_frontend_create: deriv alloc");
    layout_place(fe->dermem, layout);
    std::vector<DerivDesc> hd(3 * (size_t)S);
    for (int k = 0; k < 3 * S; k++)
        for (int l = 0; l < kMaxLevels; l++) {
            hd[k].data[l] = l < fe->nlev ? (uint32_t*)(base + dbytes * k + doff[l]) : nullptr;
            hd[k].pitch[l] = l < fe->nlev ? dpitch[l] : 0;
        }
    SVO_HIP(ctx, hipMemsetAsync(base, 0, dbytes * 3 * S, ctx->stream));  // zero borders, never rewritten
    SVO_HIP(ctx, hipMemcpyAsync(fe->d_der, hd.data(), sizeof(DerivDesc) * hd.size(), hipMemcpyHostToDevice,
                                ctx->stream));
    SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

// the host loop's state and what the switches / the detector add on the device
int create_loop_state(svo_frontend* fe) {
    svo_ctx* ctx = fe->ctx;
    const svo_frontend_config& c = fe->cfg;
    const int S = fe->S;
    fe->rs.resize(S);
    fe->pred_iters.assign(S, 0);
    fe->kf_prev.assign(S, 1);
    if (fe->sw.device_fits && hipMalloc(&fe->fit_work, sqpnp_fit_work_bytes(S)) != hipSuccess)
        return set_error(ctx, SVO_ERR_HIP, "svo_frontend_create: fit workspace");
    if (c.use_orb) {
        fe->orb = orb_batch_create(S, c.width, c.height, c.orb);
        if (!fe->orb) return set_error(ctx, SVO_ERR_ARG, "svo_frontend_create: ORB parameters or workspace");
        fe->orb_lv0.resize(S);
        fe->orb_over.assign(S, 0);
    }
    // (on the context stream: a first use of the null stream would take a fifth
    // hardware queue and serialise the step's streams)
    if (hipMalloc(&fe->score_map, fe->npx * S) != hipSuccess)
        return set_error(ctx, SVO_ERR_HIP, "svo_frontend_create: score map alloc");
    fe->pose.assign((size_t)S * 6, 0.0);
    return SVO_OK;
}

// host pool: this rank's share of the node's cores (NUMA-local to its GPU),
// at most 16 threads (the box's CPU share per GPU) and one per sequence
void create_pool(svo_frontend* fe) {
    const int world = local_world_env();
    const int rank = local_rank_env();
    int ndev = 0;
    (void)hipGetDeviceCount(&ndev);
    std::vector<int> gnode(world, -1);
    for (int r = 0; r < world && ndev > 0; r++) gnode[r] = device_numa_node(r % ndev);
    const bool pin = fe->sw.pool_pin >= 0 ? fe->sw.pool_pin == 1 : world > 1;
    if (pin) fe->host_cpus = host_cpu_plan(std::min(rank, world - 1), world, gnode.data());
    int nt = fe->cfg.host_threads > 0 ? fe->cfg.host_threads
                                      : (fe->host_cpus.empty() ? (int)std::thread::hardware_concurrency() / world
                                                               : (int)fe->host_cpus.size());
    nt = std::max(1, std::min({nt, fe->S, 16}));
    fe->pool = new Pool(nt - 1, fe->host_cpus, fe->sw.pool_spin_us);
}

int create_streams_and_events(svo_frontend* fe) {
    svo_ctx* ctx = fe->ctx;
    for (auto& e : fe->ev) (void)hipEventCreate(&e);
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    // the LK stream at the highest priority (its chain is the step's critical
    // path), the FAST stream at the lowest (FAST fills the CUs LK leaves idle
    // and the post-LK window; the speculative stereo LK behind it is ready
    // long before the keyframe needs it)
    // (the context's: created once, shared by every front end on it, svo_ctx)
    if ((!ctx->fe_lk && fe_make_stream(&ctx->fe_lk, greatest) != hipSuccess) ||
        (!ctx->fe_fast && fe_make_stream(&ctx->fe_fast, least) != hipSuccess) ||
        (!ctx->fe_copy && hipStreamCreateWithFlags(&ctx->fe_copy, hipStreamNonBlocking) != hipSuccess))
        return set_error(ctx, SVO_ERR_HIP, "svo_frontend_create: stream");
    fe->st_lk = ctx->fe_lk;
    fe->st_fast = ctx->fe_fast;
    fe->st_copy = ctx->fe_copy;
    for (hipEvent_t* e : {&fe->ev_pyr, &fe->ev_fast, &fe->ev_lk, &fe->ev_post, &fe->ev_tail, &fe->ev_stats,
                          &fe->ev_pyr_r_b[0], &fe->ev_pyr_r_b[1], &fe->ev_pre, &fe->ev_fdone, &fe->ev_full_b[0],
                          &fe->ev_full_b[1], &fe->ev_app, &fe->ev_lk2})
        (void)hipEventCreateWithFlags(e, hipEventDisableTiming);
    fe->ev_full = fe->ev_full_b[0];
    SVO_HIP(ctx, hipMemcpyAsync(fe->d_desc, fe->desc_host.data(), sizeof(PyrDesc) * fe->desc_host.size(),
                                hipMemcpyHostToDevice, ctx->stream));
    SVO_HIP(ctx, hipMemcpyAsync(fe->d_desc_r, fe->desc_r_host.data(), sizeof(PyrDesc) * fe->desc_r_host.size(),
                                hipMemcpyHostToDevice, ctx->stream));
    SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

// Let every stream finish: the inputs of the work queued ahead are about to
// change (new frames, re-init), and the caller forgets what was built from them
// (FeAhead::forget_all / forget_slot).
int fe_drain(svo_frontend* fe) {
    svo_ctx* ctx = fe->ctx;
    for (hipStream_t st : {fe->st_lk, fe->st_fast, fe->st_copy, ctx->stream, fe->up.st})
        if (st) SVO_HIP(ctx, hipStreamSynchronize(st));
    return SVO_OK;
}

int fe_set_frame(svo_frontend* fe, int seq, int t, const uint8_t* left, const uint8_t* right, int stride, bool bgr) {
    if (!fe || seq < 0 || seq >= fe->S || t < 0 || t >= fe->T || !left || !right ||
        stride < (bgr ? 3 : 1) * fe->raw_w)
        return SVO_ERR_ARG;
    svo_ctx* ctx = fe->ctx;
    fe->fed = true;
    int rd = fe_drain(fe);
    if (rd) return rd;
    fe->ahead.forget_slot(t, fe->T);  // built from / detected on the old image
    // the slot now holds frame t, resident (the drain above finished any streamed
    // upload into it): steps keep finding it in the ring
    if (!fe->up.t.empty()) {
        fe->up.t[t] = t;
        fe->up.free_rec[t] = 0;
    }
    if (fe->rect[0]) {
        // raw frames: each eye's bytes into the staging pair, rectified from there into
        // the slot's level 0 with that eye's maps (raw frames are not kept)
        const size_t bytes = (size_t)(fe->raw_h - 1) * stride + (size_t)(bgr ? 3 : 1) * fe->raw_w;
        if (bytes > fe->rect_cap) {
            if (fe->rect_stage) SVO_HIP(ctx, hipFree(fe->rect_stage));
            fe->rect_stage = nullptr;
            fe->rect_cap = 0;
            SVO_HIP(ctx, hipMalloc((void**)&fe->rect_stage, 2 * bytes));
            fe->rect_cap = bytes;
        }
        for (int side = 0; side < 2; side++) {
            uint8_t* dst = fe->rect_stage + (size_t)side * fe->rect_cap;
            SVO_HIP(ctx, hipMemcpyAsync(dst, side ? right : left, bytes, hipMemcpyHostToDevice, ctx->stream));
            const PyrDesc* d = (side ? fe->d_desc_r : fe->d_desc) + (size_t)t * fe->S + seq;
            SVO_HIP(ctx, launch_rectify_batched(dst, 0, stride, fe->rect[side]->dev, d, 1, bgr, ctx->stream));
        }
        SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return SVO_OK;
    }
    for (int side = 0; side < 2; side++) {
        svo_image* im = (side ? fe->frames_r : fe->frames)[(size_t)seq * fe->T + t];
        const uint8_t* px = side ? right : left;
        uint8_t* l0 = const_cast<uint8_t*>(im->desc.lv[0].data);
        if (bgr) {
            int rc = ingest_bgr(ctx, px, stride, fe->W, fe->H, l0, im->desc.lv[0].pitch);
            if (rc) return rc;
        } else {
            SVO_HIP(ctx, hipMemcpy2DAsync(l0, im->desc.lv[0].pitch, px, stride, fe->W, fe->H, hipMemcpyHostToDevice,
                                          ctx->stream));
        }
    }
    SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

}  // namespace

extern "C" {

int svo_frontend_create(svo_ctx* ctx, const svo_frontend_config* cfg, svo_frontend** out) {
    if (!ctx || !cfg || !out) return SVO_ERR_ARG;
    const svo_frontend_config& c = *cfg;
    if (c.width <= 0 || c.height <= 0 || c.n_seq <= 0 || c.n_frames < 2 || c.n_features <= 0 || c.max_level < 0 ||
        !lk_supported(c.win, c.win) || c.stereo_win <= 2 || c.stereo_max_level < 0 ||
        !lk_supported(c.stereo_win, c.stereo_win) || c.pnp_iterations <= 0 ||
        !(c.pnp_confidence > 0 && c.pnp_confidence < 1) ||
        (c.keyframe_rule != SVO_KF_EVERY && c.keyframe_rule != SVO_KF_REFERENCE) ||
        (c.bucket_size > 0 && (c.per_bucket <= 0 || c.width / c.bucket_size <= 0)) ||
        (c.use_orb != 0 && c.use_orb != 1) || (c.use_orb && c.bucket_size > 0))
        return set_error(ctx, SVO_ERR_ARG, "svo_frontend_create: bad config");
    // (every failure below returns through the guard, which destroys what exists so far)
    std::unique_ptr<svo_frontend, void (*)(svo_frontend*)> guard(new svo_frontend(), svo_frontend_destroy);
    svo_frontend* fe = guard.get();
    fe->ctx = ctx;
    fe->cfg = c;
    fe->sw = fe_read_switches(c);
    create_sizes(fe);
    fe->raw_w = fe->W;
    fe->raw_h = fe->H;
    for (auto part : {create_frames, create_device_state, create_pinned_mirrors, create_coherent,
                      create_deriv_pyramids, create_loop_state}) {
        int rc = part(fe);
        if (rc) return rc;
    }
    create_pool(fe);
    int rc = create_streams_and_events(fe);
    if (rc) return rc;
    *out = guard.release();
    return SVO_OK;
}

void svo_frontend_destroy(svo_frontend* fe) {
    if (!fe) return;
    if (fe->ctx) (void)hipStreamSynchronize(fe->ctx->stream);
    // (the streams are the context's: finished here, destroyed with the context)
    for (hipStream_t st : {fe->st_lk, fe->st_fast, fe->st_copy, fe->up.st})
        if (st) (void)hipStreamSynchronize(st);
    delete fe->pool;
    for (auto* v : {&fe->frames, &fe->frames_r})
        for (auto* f : *v)
            if (f) svo_image_destroy(fe->ctx, f);
    if (fe->dmem) (void)hipFree(fe->dmem);
    if (fe->dermem) (void)hipFree(fe->dermem);
    if (fe->hmem) (void)hipHostFree(fe->hmem);
    if (fe->zmem) (void)hipHostFree(fe->zmem);
    if (fe->zout) (void)hipHostFree(fe->zout);
    for (auto& e : fe->ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {fe->ev_pyr, fe->ev_fast, fe->ev_lk, fe->ev_post, fe->ev_tail, fe->ev_stats, fe->ev_pyr_r_b[0],
                         fe->ev_pyr_r_b[1], fe->ev_pre, fe->ev_fdone, fe->ev_full_b[0], fe->ev_full_b[1], fe->ev_app,
                         fe->ev_lk2})
        if (e) (void)hipEventDestroy(e);
    if (fe->score_map) (void)hipFree(fe->score_map);
    for (hipEvent_t e : fe->up.ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : fe->up.ev_free)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : fe->ev_trk)
        if (e) (void)hipEventDestroy(e);
    if (fe->trk_mem) (void)hipFree(fe->trk_mem);
    fe_places_destroy(fe);
    if (fe->up.stage) (void)hipFree(fe->up.stage);
    if (fe->rect_stage) (void)hipFree(fe->rect_stage);
    orb_batch_destroy(fe->orb);
    if (fe->fit_work) (void)hipFree(fe->fit_work);
    if (fe->win.mem) (void)hipFree(fe->win.mem);
    if (fe->win.h_pose) (void)hipHostFree(fe->win.h_pose);
    delete fe;
}

int svo_frontend_set_frame(svo_frontend* fe, int seq, int t, const uint8_t* left, const uint8_t* right, int stride) {
    return fe_set_frame(fe, seq, t, left, right, stride, false);
}

int svo_frontend_set_frame_bgr(svo_frontend* fe, int seq, int t, const uint8_t* left_bgr, const uint8_t* right_bgr,
                               int stride) {
    return fe_set_frame(fe, seq, t, left_bgr, right_bgr, stride, true);
}

int svo_frontend_set_rectification(svo_frontend* fe, const svo_rect_maps* left, const svo_rect_maps* right) {
    if (!fe || !left || !right) return SVO_ERR_ARG;
    svo_ctx* ctx = fe->ctx;
    if (fe->fed || fe->rect[0])
        return set_error(ctx, SVO_ERR_ARG, "svo_frontend_set_rectification: once, before the first set_frame, "
                                           "queue_frames or init");
    for (const svo_rect_maps* m : {left, right})
        if (m->dev.w != fe->W || m->dev.h != fe->H)
            return set_error(ctx, SVO_ERR_ARG, "svo_frontend_set_rectification: maps of %d x %d, config %d x %d",
                             m->dev.w, m->dev.h, fe->W, fe->H);
    if (left->dev.raw_w != right->dev.raw_w || left->dev.raw_h != right->dev.raw_h)
        return set_error(ctx, SVO_ERR_ARG, "svo_frontend_set_rectification: the eyes' raw sizes differ");
    fe->rect[0] = left;
    fe->rect[1] = right;
    fe->raw_w = left->dev.raw_w;
    fe->raw_h = left->dev.raw_h;
    return SVO_OK;
}

int svo_frontend_set_stereo_matcher(svo_frontend* fe, const svo_stereo_rows_params* params) {
    if (!fe || !params) return SVO_ERR_ARG;
    svo_ctx* ctx = fe->ctx;
    if (fe->fed || fe->rows_on)
        return set_error(ctx, SVO_ERR_ARG, "svo_frontend_set_stereo_matcher: once, before the first set_frame, "
                                           "queue_frames or init");
    if (!stereo_rows_params_ok(*params))
        return set_error(ctx, SVO_ERR_ARG, "svo_frontend_set_stereo_matcher: parameters out of range");
    fe->rows = *params;
    fe->rows_on = true;
    return SVO_OK;
}

int svo_frontend_set_stereo_tracking(svo_frontend* fe, const svo_stereo_rows_params* params, int guide) {
    if (!fe || !params) return SVO_ERR_ARG;
    svo_ctx* ctx = fe->ctx;
    if (!fe->win.ring.ur)
        return set_error(ctx, SVO_ERR_ARG, "svo_frontend_set_stereo_tracking: no stereo window enabled");
    if (fe->ahead.stepped >= 0 || fe->trk_on)
        return set_error(ctx, SVO_ERR_ARG, "svo_frontend_set_stereo_tracking: once, after "
                                           "svo_frontend_window_enable_stereo and before svo_frontend_init");
    if (!stereo_rows_params_ok(*params) || guide < 0 || guide > 15)
        return set_error(ctx, SVO_ERR_ARG, "svo_frontend_set_stereo_tracking: parameters out of range "
                                           "(svo_stereo_match_rows', guide 0..15)");
    const size_t n = (size_t)fe->S * fe->CAP;
    auto layout = [&](Carver& p) {
        fe->trk_prior = p.take<int>(n);
        fe->trk_n = p.take<int>(fe->S);
        fe->trk_next = p.take<float>(2 * n);
        fe->trk_status = p.take<uint8_t>(n);
    };
    const size_t bytes = layout_bytes(layout);
    SVO_HIP(ctx, hipMalloc(&fe->trk_mem, bytes));
    layout_place(fe->trk_mem, layout);
    SVO_HIP(ctx, hipMemsetAsync(fe->trk_mem, 0, bytes, ctx->stream));
    SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    fe->ev_trk.assign(fe->T, nullptr);
    for (auto& e : fe->ev_trk) SVO_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    fe->trk_rec.assign(fe->T, 0);
    fe->trk = *params;
    fe->trk_guide = guide;
    fe->trk_on = true;
    return SVO_OK;
}

int svo_frontend_queue_frames(svo_frontend* fe, int t, const uint8_t* const* left, const uint8_t* const* right,
                              int stride, int bgr) {
    if (!fe || t < 0 || !left || !right || stride < (bgr ? 3 : 1) * fe->raw_w) return SVO_ERR_ARG;
    svo_ctx* ctx = fe->ctx;
    FeUpload& up = fe->up;
    // (W x H: the host frames' size -- the raw frames' once rectification is set)
    const int S = fe->S, T = fe->T, W = fe->raw_w, H = fe->raw_h;
    if (T < 4) return set_error(ctx, SVO_ERR_ARG, "svo_frontend_queue_frames: needs a ring of n_frames >= 4");
    for (int s = 0; s < S; s++)
        if (!left[s] || !right[s]) return SVO_ERR_ARG;
    fe->fed = true;
    // ring discipline: frame t's pyramid is built at the end of step t - 2, so it is
    // queued before that step (t >= stepped + 3); its slot's previous frame t - T is
    // no longer read once step t - T + 1 returned (t <= stepped + T - 1)
    // a frame at or before the last step restarts the loop: everything queued and
    // built ahead is finished and forgotten, and the window opens as before init
    const int stepped = fe->ahead.stepped;
    if (stepped >= 0 && t <= stepped) {
        int rd = fe_drain(fe);
        if (rd) return rd;
        fe->ahead.forget_all();
        std::fill(up.t.begin(), up.t.end(), -1);
        std::fill(up.free_rec.begin(), up.free_rec.end(), 0);
    } else if (stepped >= 0 && (t < stepped + 3 || t > stepped + T - 1)) {
        return set_error(ctx, SVO_ERR_ARG, "svo_frontend_queue_frames: frame outside the ring window "
                                           "(stepped + 3 .. stepped + n_frames - 1)");
    }
    if (up.t.empty()) {
        if (!ctx->fe_up) SVO_HIP(ctx, hipStreamCreateWithFlags(&ctx->fe_up, hipStreamNonBlocking));
        up.st = ctx->fe_up;
        up.ev.assign(T, nullptr);
        for (auto& e : up.ev) SVO_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        up.t.assign(T, -1);
        up.ev_free.assign(T, nullptr);
        for (auto& e : up.ev_free) SVO_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        up.free_rec.assign(T, 0);
    }
    // the staging block mirrors the host frames (rows `stride` apart, sequences
    // H rows apart): a run of sequences whose buffers follow each other in memory
    // is one contiguous H2D copy; grown (after the queued uploads) for a wider stride
    const size_t seq_bytes = (size_t)H * stride;
    if (seq_bytes > up.cap) {
        SVO_HIP(ctx, hipStreamSynchronize(up.st));
        if (up.stage) SVO_HIP(ctx, hipFree(up.stage));
        up.stage = nullptr;
        up.cap = seq_bytes;
        SVO_HIP(ctx, hipMalloc(&up.stage, 2 * (size_t)S * up.cap));
    }
    up.seq = seq_bytes;  // (the conversion of earlier queued frames captured their own stride)
    up.stride = stride;
    up.bgr = bgr != 0;
    const int slot = t % T;
    const size_t last_row = (size_t)(bgr ? 3 : 1) * W;  // bytes of a frame's last row (no stride padding after it)
    // the slot's previous frame (t - T) is last read by LK(t - T + 1): the copy into
    // the slot waits for it on the device, not only by the host's window above
    if (up.free_rec[slot]) SVO_HIP(ctx, hipStreamWaitEvent(up.st, up.ev_free[slot], 0));
    up.free_rec[slot] = 0;
    // ... and, with svo_frontend_set_stereo_tracking, by the guided match of that
    // frame's tracked features behind its keyframe (fe_track_stereo)
    if (fe->trk_on && fe->trk_rec[slot]) SVO_HIP(ctx, hipStreamWaitEvent(up.st, fe->ev_trk[slot], 0));
    if (fe->trk_on) fe->trk_rec[slot] = 0;
    // ... and, with svo_frontend_places_enable, by the describe pass of that frame's record
    if (fe->pl.slots && fe->pl.img_rec[slot]) SVO_HIP(ctx, hipStreamWaitEvent(up.st, fe->pl.ev_img[slot], 0));
    if (fe->pl.slots) fe->pl.img_rec[slot] = 0;
    for (int side = 0; side < 2; side++) {
        const uint8_t* const* src = side ? right : left;
        uint8_t* dst = up.stage + (size_t)side * S * up.cap;
        for (int s0 = 0; s0 < S;) {
            int s1 = s0 + 1;
            while (s1 < S && src[s1] == src[s1 - 1] + seq_bytes) s1++;
            const size_t n = (size_t)(s1 - s0 - 1) * up.seq + (size_t)(H - 1) * stride + last_row;
            SVO_HIP(ctx, hipMemcpyAsync(dst + (size_t)s0 * up.seq, src[s0], n, hipMemcpyHostToDevice, up.st));
            s0 = s1;
        }
        const PyrDesc* d = (side ? fe->d_desc_r : fe->d_desc) + (size_t)slot * S;
        if (fe->rect[side])  // raw frames: the same stage with the eye's gather in front
            SVO_HIP(ctx, launch_rectify_batched(dst, up.seq, stride, fe->rect[side]->dev, d, S, bgr != 0, up.st));
        else
            SVO_HIP(ctx, launch_ingest_batched(dst, up.seq, stride, d, S, W, H, bgr != 0, up.st));
    }
    SVO_HIP(ctx, hipEventRecord(up.ev[slot], up.st));
    up.t[slot] = t;
    fe->ahead.forget_slot(slot, T);  // anything built ahead from the slot's previous frame is stale
    return SVO_OK;
}

int svo_frontend_upload_wait(svo_frontend* fe, int t) {
    if (!fe || t < 0) return SVO_ERR_ARG;
    if (fe->up.t.empty() || fe->up.t[t % fe->T] != t) return SVO_OK;
    SVO_HIP(fe->ctx, hipEventSynchronize(fe->up.ev[t % fe->T]));
    return SVO_OK;
}

int svo_frontend_prebuild_pyramids(svo_frontend* fe) {
    if (!fe) return SVO_ERR_ARG;
    for (int t = 0; t < fe->T; t++) {
        if (!fe->up.t.empty() && fe->up.t[t] >= 0) SVO_HIP(fe->ctx, hipStreamWaitEvent(fe->ctx->stream, fe->up.ev[t], 0));
        SVO_HIP(fe->ctx, launch_pyramid_batched(fe->d_desc + (size_t)t * fe->S, fe->S, fe->W, fe->H, fe->nlev,
                                                fe->ctx->stream));
        SVO_HIP(fe->ctx, launch_pyramid_batched(fe->d_desc_r + (size_t)t * fe->S, fe->S, fe->W, fe->H, fe->nlev,
                                                fe->ctx->stream));
    }
    SVO_HIP(fe->ctx, hipStreamSynchronize(fe->ctx->stream));
    return SVO_OK;
}

// Tracking::startStereo's first frame (R:src/tracking.cpp:233-235): extractFeatures
// (FAST without a mask: prevFrame == frame has no features yet), stereo match,
// triangulation with the identity pose (Frame's default), capped at n_features.
// Frame t0 is a keyframe under either rule (nextFrame: lastFrameID == 0).
int svo_frontend_init(svo_frontend* fe, int t0) {
    if (!fe || t0 < 0) return SVO_ERR_ARG;
    fe->fed = true;
    int rd = fe_drain(fe);
    if (rd) return rd;
    fe->ahead.forget_all();
    svo_ctx* ctx = fe->ctx;
    const int S = fe->S;
    for (int s = 0; s < S; s++) fe->h_target[s] = fe->cfg.n_features;
    std::fill(fe->kf_prev.begin(), fe->kf_prev.end(), 1);
    const PyrDesc* dcur = fe->d_desc + (size_t)(t0 % fe->T) * S;
    {
        int rw = fe_wait_upload(fe, t0, ctx->stream);
        if (rw) return rw;
    }
    SVO_HIP(ctx, launch_pyramid_scharr_batched(dcur, fe->d_der + (size_t)(t0 % 3) * S, S, fe->W, fe->H, fe->nlev,
                                               ctx->stream));
    SVO_HIP(ctx, launch_pyramid_batched(fe->d_desc_r + (size_t)(t0 % fe->T) * S, S, fe->W, fe->H, fe->nlev,
                                        ctx->stream));
    SVO_HIP(ctx, hipEventRecord(fe->ev_pyr_r_b[t0 & 1], ctx->stream));
    SVO_HIP(ctx, hipMemsetAsync(fe->nA, 0, sizeof(int) * S, ctx->stream));
    SVO_HIP(ctx, hipMemsetAsync(fe->map_n, 0, sizeof(int) * S, ctx->stream));
    SVO_HIP(ctx, hipMemsetAsync(fe->pend_n, 0, sizeof(int) * S, ctx->stream));
    if (fe->win.slots) SVO_HIP(ctx, hipMemsetAsync(fe->win.ring.map_epoch, 0, sizeof(int) * S, ctx->stream));
    int rc = fe->orb ? fe_orb_detect(fe, t0, false, ctx->stream) : fe_fast_and_bucket(fe, dcur, false, ctx->stream);
    if (rc) return rc;
    // n_in = nA (zero): nothing to compact, the candidates fill the set; no statistics
    rc = fe_keyframe(fe, t0, fe->nA, nullptr, fe->xyA, fe->midA, fe->cfg.n_features, ctx->stream, -1);
    if (rc) return rc;
    // the window starts over with frame t0 (its map ids start from 0 again)
    fe->win.count = 0;
    rc = fe_window_record(fe, t0, ctx->stream);
    if (rc) return rc;
    fe_places_restart(fe, t0);
    rc = fe_places_record(fe, t0, ctx->stream);
    if (rc) return rc;
    for (int s = 0; s < S; s++) fe_set_pose(fe, s, false, nullptr, nullptr);
    SVO_HIP(ctx, launch_finalize_map(fe_pending(fe), S, ctx->stream));
    rc = fe_places_flush(fe, ctx->stream);
    if (rc) return rc;
    SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ph_collect(fe);
    std::fill(fe->pose.begin(), fe->pose.end(), 0.0);
    fe->ahead.stepped = t0;
    return SVO_OK;
}

}  // extern "C"
