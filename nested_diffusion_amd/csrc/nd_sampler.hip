// nd_sampler.hip -- what runs on the ensemble handle (nd_handle.hpp): the encoder hoist, the per-member entry points, the hipGraph
// that replays a whole p_sample_loop and the graph of a whole test batch.  The step kernels: csrc/nd_step.hip.  gfx950 only.
//
// Reference path (file:line relative to the reference checkout):
//   diffusion/diffusion_utils.py:133-163   p_sample_loop
//   diffusion/diffusion_utils.py:54-111    p_sample / p_sample_t_1to0
#include "nd_handle.hpp"
#include "nd_cond_gemm.hpp"
#include "nd_persist.hpp"
#include "nd_rng.hpp"

#include <cstring>
#include <cstdlib>

template <int MODE>
static hipError_t launch_skinny(const SkinnyDesc* table, int K, int N, int M, int t, int nm, int half, hipStream_t st) {
    return nd_launch_skinny(nd_skinny_launch<MODE>(K, N, M, nm, half), SkinnyDesc{}, table, nm, M, t, st);
}

// One ConditionalLinear block (MODE 0: lin2, MODE 1: lin3 + lin4 projection) for nm members: the weight-streaming kernel for
// small row counts, the LDS-tiled kernel above 128 rows (nd_cond_gemm.hpp).  Returns the partial-sum count per (row, class)
// the MODE 1 form leaves in epart.
static int step_partials(const nd_handle_s* h, int M) {
    const int F = h->cfg.feature_dim;
    const CondGemmPlan p = nd_cond_gemm_plan(F, F, M, 1, h->half);
    return p.use_tile ? p.ntl : h->NT;
}

template <int MODE>
static hipError_t launch_step_block(nd_handle_s* h, const SkinnyDesc* table, int M, int t, int nm, hipStream_t st) {
    const int F = h->cfg.feature_dim;
    const CondGemmPlan p = nd_cond_gemm_plan(F, F, M, nm, h->half);
    if (p.use_tile) return nd_launch_cond_gemm(MODE, p, SkinnyDesc{}, table, M, t, h->tile_ws, st);
    return launch_skinny<MODE>(table, F, F, M, t, nm, h->half, st);
}

// "The inputs of this batch have been read": count the call on the device and publish the count to the caller's host-visible word
// (system-scope store: the word lives in pinned host memory).  Enqueued by nd_predict_batch right behind the LAST kernel that reads
// images_dev, so a loader may refill that buffer for the next batch while this batch's sampler is still running.
__global__ void k_inputs_consumed(unsigned* seq, unsigned* flag) {
    const unsigned v = *seq + 1u;
    *seq = v;
    __hip_atomic_store(flag, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

static int encode_impl(nd_handle h, int m0, int nm, const float* x_dev, int B, void* stream, bool signal_inputs) {
    int rc = nd_check_range(h, m0, nm);
    if (rc != ND_OK) return rc;
    if (!x_dev) return nd_set_err(ND_ERR_ARG, "x_dev is NULL");
    if (B < 1 || B > h->cfg.max_batch) return nd_set_err(ND_ERR_ARG, "B=%d outside [1,%d]", B, h->cfg.max_batch);
    hipStream_t st = (hipStream_t)stream;
    const nd_config& c = h->cfg;
    const int K = c.n_members, H = c.hidden_dim, F = c.feature_dim, D = c.data_dim;
    nd_launch_pack(x_dev, h->xpack, B, D, h->half, st);    // images -> frag16 once; every member reads the same batch
    if (signal_inputs && h->input_flag)                    // nd_predict_batch: x_dev (= images_dev) is not read again by this call
        hipLaunchKernelGGL(k_inputs_consumed, dim3(1), dim3(1), 0, st, h->input_seq, h->input_flag);
    if (h->enc_splitk) {
        const SkinnyLaunch L = nd_skinny_launch<2>(D, H, B, nm, h->half);
        HIP_CHECK(nd_launch_skinny(L, SkinnyDesc{}, h->spk_dev + m0, nm, B, 0, st));
        nd_launch_splitk_epilogue(SplitKEpiDesc{}, h->spke_dev + m0, nm, B, H, L.S, st);
    } else {
        HIP_CHECK(launch_skinny<0>(h->descs_dev + (size_t)L_ENC0 * K + m0, D, H, B, 0, nm, h->half, st));
    }
    HIP_CHECK(launch_skinny<0>(h->descs_dev + (size_t)L_ENC1 * K + m0, H, H, B, 0, nm, h->half, st));
    HIP_CHECK(launch_skinny<0>(h->descs_dev + (size_t)L_ENC2 * K + m0, H, F, B, 0, nm, h->half, st));
    HIP_CHECK(hipGetLastError());
    h->encoded_B = B;
    return ND_OK;
}

extern "C" int nd_encode(nd_handle h, int m0, int nm, const float* x_dev, int B, void* stream) {
    return encode_impl(h, m0, nm, x_dev, B, stream, false);
}

extern "C" int nd_set_loop_form(nd_handle h, int mode, float skew_us) {
    if (!h) return nd_set_err(ND_ERR_ARG, "handle is NULL");
    if (mode != 0 && mode != 1) return nd_set_err(ND_ERR_ARG, "mode must be 0 (per-step kernels) or 1 (one launch per loop)");
    if (skew_us > 1e6f) return nd_set_err(ND_ERR_ARG, "skew_us out of range");
    h->persist_mode = mode;
    if (skew_us >= 0.f) h->persist_skew_ticks = (int)(skew_us * 100.0f);
    nd_drop_graphs(h);
    return ND_OK;
}

extern "C" int nd_loop_form(nd_handle h) { return h && h->persist_last ? 1 : 0; }

extern "C" int nd_persist_status(nd_handle h, int reset) {
    if (!h || !h->ws) return nd_set_err(ND_ERR_STATE, "workspace not bound");
    HIP_CHECK(hipDeviceSynchronize());
    unsigned flag = 0;
    HIP_CHECK(hipMemcpy(&flag, h->persist_bar + ND_PERSIST_ERR_WORD, sizeof flag, hipMemcpyDeviceToHost));
    if (reset && flag) HIP_CHECK(hipMemset(h->persist_bar, 0, ND_PERSIST_BAR_WORDS * sizeof(unsigned)));   // counters of the abandoned launch too
    return flag ? 1 : 0;
}

// event-record nodes of a graph about to be instantiated (-1 if the graph cannot be walked)
static int count_event_record_nodes(hipGraph_t g) {
    size_t n = 0;
    if (hipGraphGetNodes(g, nullptr, &n) != hipSuccess) return -1;
    std::vector<hipGraphNode_t> nodes(n);
    if (n && hipGraphGetNodes(g, nodes.data(), &n) != hipSuccess) return -1;
    int cnt = 0;
    for (size_t i = 0; i < n; ++i) {
        hipGraphNodeType ty;
        if (hipGraphNodeGetType(nodes[i], &ty) != hipSuccess) return -1;
        if (ty == hipGraphNodeTypeEventRecord) ++cnt;
    }
    return cnt;
}

extern "C" int nd_profile_probe_nodes(nd_handle h) {
    if (!h) return nd_set_err(ND_ERR_ARG, "handle is NULL");
    return h->probe_nodes;
}

extern "C" int nd_profile_read(nd_handle h, float* out_us, int* n_samples) {
    if (!h || !out_us || !n_samples) return nd_set_err(ND_ERR_ARG, "NULL argument");
    double acc[3] = {0, 0, 0};
    const int n = h->probe_steps;
    for (int s = 0; s < n; ++s)
        for (int k = 0; k < 3; ++k) {
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, h->probe_events[4 * s + k], h->probe_events[4 * s + k + 1]));
            acc[k] += ms * 1000.0;
        }
    out_us[0] = n ? (float)(acc[0] / n) : 0.f;      // head(i) interval              = head + o
    out_us[1] = n ? (float)(acc[1] / n) : 0.f;      // lin2 + lin3 (i) interval      = 2 blocks + o   (both launches, one record node)
    out_us[2] = n ? (float)(acc[2] / n) : 0.f;      // whole step i+1 interval       = head + 2 blocks + o
    const float head = out_us[2] - out_us[1];       // the head alone: the record overheads of the two intervals cancel
    out_us[3] = n ? (out_us[0] - head > 0.f ? out_us[0] - head : 0.f) : 0.f;     // o: what a record node adds to a loaded interval
    *n_samples = n;
    return ND_OK;
}

// The row checks of every entry point that runs the loop, in this order: B, mc and B*mc, T, schedule[, the encoder hoist's B].
static int check_rows(nd_handle_s* h, int B, int mc, int T, bool need_encoded = true) {
    if (B < 1 || B > h->cfg.max_batch) return nd_set_err(ND_ERR_ARG, "B=%d outside [1,%d]", B, h->cfg.max_batch);
    if (mc < 1 || mc > 65535 || (long)B * mc > h->cfg.max_rows)
        return nd_set_err(ND_ERR_ARG, "mc=%d outside [1,65535] or B*mc=%ld exceeds max_rows=%d", mc, (long)B * mc, h->cfg.max_rows);
    if (T < 1 || T > h->cfg.n_steps) return nd_set_err(ND_ERR_ARG, "T=%d outside [1,%d]", T, h->cfg.n_steps);
    if (h->sched_T < T) return nd_set_err(ND_ERR_STATE, "schedule holds %d steps, need %d (nd_set_schedule)", h->sched_T, T);
    if (need_encoded && h->encoded_B != B) return nd_set_err(ND_ERR_STATE, "nd_encode ran with B=%d, sampling asks B=%d", h->encoded_B, B);
    return ND_OK;
}

// With a sampler plan set (nd_set_sampler) the loop runs the plan's S steps: the entry points that run the loop take T == S only.
static int check_plan(const nd_handle_s* h, int T) {
    const int S = (int)h->plan_tau.size();
    if (S && T != S) return nd_set_err(ND_ERR_STATE, "sampler plan holds S=%d steps, the call asks T=%d (nd_set_sampler)", S, T);
    return ND_OK;
}

// Which operand layout emit_loop picks for the step blocks of a launch over nm members at M rows (its `b9`): the frag32b3 images on the
// bf16 matrix pipe above 128 rows where the handle holds them and the descriptors travel by value.  Recorded per member at every entry
// point that runs the loop (graph replays included: the choice is a function of the call's shape) so that nd_member_buffer reads the
// copies the last launch really wrote.
static bool loop_writes_split(const nd_handle_s* h, int M, int nm) {
    return h->b9 && nm <= ND_INLINE_DESCS && nd_cond_gemm_plan(h->cfg.feature_dim, h->cfg.feature_dim, M, nm, h->half).use_tile;
}

// The argument lists of the step head (both forms) and of the last step (nd_step.hpp), packed for hipLaunchKernel / a kernel node;
// both copy the values when they are called, so one record serves every step of a loop.
struct HeadArgs {
    MemberInline mi; const MemberDev* members; StepIO io;
    int mode, i_step, t_prev, t, B, M, maxM, F, NT, T;
    void* p[13];
    void** ptrs() {
        void* q[13] = {&mi, &members, &io, &mode, &i_step, &t_prev, &t, &B, &M, &maxM, &F, &NT, &T};
        return (void**)memcpy(p, q, sizeof p);
    }
};
struct FinalArgs {
    MemberInline mi; const MemberDev* members; StepIO io;
    int eps_only, par_cur, B, M, maxM, NT, T;
    float* eps_out; size_t eps_ms;
    void* p[12];
    void** ptrs() {
        void* q[12] = {&mi, &members, &io, &eps_only, &par_cur, &B, &M, &maxM, &NT, &T, &eps_out, &eps_ms};
        return (void**)memcpy(p, q, sizeof p);
    }
};

// head -> lin2 -> lin3 for one member, then `final` in the requested mode (1 eps, 2 p_sample, 3 1to0)
static int single_eval(nd_handle_s* h, int member, StepIO io, int t, int final_mode, float* out, int B, int mc, hipStream_t st) {
    const nd_config& c = h->cfg;
    const int K = c.n_members, F = c.feature_dim, C = c.y_dim, M = B * mc, NT = step_partials(h, M);
    nd_note_h_layout(h, member, 1, false);        // the per-member entry points always run the frag16 / frag32h forms into h1 / h2
    HeadArgs ha{MemberInline{}, h->members_dev + member, io, ND_HEAD_GIVEN, 0, 0, t, B, M, c.max_rows, F, NT, c.n_steps};
    HIP_CHECK(hipLaunchKernel(nd_step_head_kernel(C, false), dim3((F + 1023) / 1024, M, 1), dim3(256), ha.ptrs(), 0, st));
    HIP_CHECK(launch_step_block<0>(h, h->descs_dev + (size_t)L_LIN2 * K + member, M, t, 1, st));
    HIP_CHECK(launch_step_block<1>(h, h->descs_dev + (size_t)L_LIN3 * K + member, M, t, 1, st));
    FinalArgs fa{MemberInline{}, h->members_dev + member, io, final_mode, t, B, M, c.max_rows, NT, c.n_steps, out, 0};
    HIP_CHECK(hipLaunchKernel(nd_step_final_kernel(C), dim3(M, 1, 1), dim3(64), fa.ptrs(), 0, st));
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_eps_theta(nd_handle h, int member, const float* y_dev, const float* yhat_dev, int t, float* eps_out, int B,
                            int mc, void* stream) {
    int rc = nd_check_range(h, member, 1);
    if (rc != ND_OK) return rc;
    if (!y_dev || !yhat_dev || !eps_out) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (B < 1 || B > h->cfg.max_batch || mc < 1 || (long)B * mc > h->cfg.max_rows) return nd_set_err(ND_ERR_ARG, "B/mc out of range");
    if (t < 0 || t >= h->cfg.n_steps) return nd_set_err(ND_ERR_ARG, "t=%d outside [0,%d)", t, h->cfg.n_steps);
    if (h->encoded_B != B) return nd_set_err(ND_ERR_STATE, "nd_encode ran with B=%d, asked B=%d", h->encoded_B, B);
    StepIO io{};
    io.yhat = yhat_dev; io.y_in = y_dev; io.alphas = h->alphas; io.omabs = h->omabs;
    return single_eval(h, member, io, t, 1, eps_out, B, mc, (hipStream_t)stream);
}

extern "C" int nd_p_sample(nd_handle h, int member, const float* y_dev, const float* yhat_dev, const float* ymean_dev,
                           const float* z_dev, int t, float* y_out, int B, int mc, void* stream) {
    int rc = nd_check_range(h, member, 1);
    if (rc != ND_OK) return rc;
    if (!y_dev || !yhat_dev || !ymean_dev || !y_out) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (t < 0) return nd_set_err(ND_ERR_ARG, "t must be >= 0");
    if (t > 0 && !z_dev) return nd_set_err(ND_ERR_ARG, "z_dev is required for t >= 1");
    rc = check_rows(h, B, mc, t + 1);
    if (rc != ND_OK) return rc;
    StepIO io{};
    io.yhat = yhat_dev; io.ymean = ymean_dev; io.y_in = y_dev; io.noise = z_dev; io.alphas = h->alphas; io.omabs = h->omabs;
    return single_eval(h, member, io, t, t > 0 ? 2 : 3, y_out, B, mc, (hipStream_t)stream);
}

// Enqueue (eager) or record (graph) the 3T+1 kernels of one p_sample_loop for a member range.
struct Emitter {
    hipStream_t st;
    hipGraph_t graph = nullptr;
    hipGraphNode_t last = nullptr;
    hipError_t err = hipSuccess;
    bool capturing = false;          // st is being captured into a graph (nd_predict_batch)
    void record(hipEvent_t ev) {
        if (err != hipSuccess) return;
        if (!graph && capturing) {
            // Under stream capture a plain hipEventRecord only orders the captured work: nothing would stamp the event when the
            // graph is replayed.  Put an event-record NODE into the graph being captured, behind the stream's current dependency
            // set, and make it the stream's new dependency set (hipEventRecordWithFlags(..., hipEventRecordExternal) is the short
            // form of this, but returns hipErrorInvalidValue under relaxed-mode capture on ROCm 7.2).
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            unsigned long long id = 0;
            hipGraph_t g = nullptr;
            const hipGraphNode_t* deps = nullptr;
            size_t ndeps = 0;
            err = hipStreamGetCaptureInfo_v2(st, &cs, &id, &g, &deps, &ndeps);
            if (err != hipSuccess) return;
            if (cs != hipStreamCaptureStatusActive || !g) { err = hipErrorStreamCaptureInvalidated; return; }
            hipGraphNode_t node;
            err = hipGraphAddEventRecordNode(&node, g, deps, ndeps, ev);
            if (err != hipSuccess) return;
            err = hipStreamUpdateCaptureDependencies(st, &node, 1, hipStreamSetCaptureDependencies);
        } else if (!graph) {
            err = hipEventRecord(ev, st);
        } else {
            hipGraphNode_t node;
            err = hipGraphAddEventRecordNode(&node, graph, last ? &last : nullptr, last ? 1 : 0, ev);
            last = node;
        }
    }
    void emit(void* fn, dim3 grid, dim3 block, void** args, size_t lds = 0) {
        if (err != hipSuccess) return;
        if (!graph) {
            err = hipLaunchKernel(fn, grid, block, args, lds, st);
        } else {
            hipKernelNodeParams p{};
            p.func = fn; p.gridDim = grid; p.blockDim = block; p.sharedMemBytes = (unsigned)lds; p.kernelParams = args; p.extra = nullptr;
            hipGraphNode_t node;
            err = hipGraphAddKernelNode(&node, graph, last ? &last : nullptr, last ? 1 : 0, &p);
            last = node;
        }
    }
};

// make the handle hold at least n probe events (false: an event could not be created)
static bool grow_probe_events(nd_handle_s* h, size_t n) {
    const size_t old = h->probe_events.size();
    if (old < n) h->probe_events.resize(n);
    for (size_t e = old; e < n; ++e)
        if (hipEventCreate(&h->probe_events[e]) != hipSuccess) return false;
    return true;
}

static hipError_t emit_loop(nd_handle_s* h, Emitter& em, int m0, int nm, StepIO io, int B, int mc, int T) {
    const nd_config& c = h->cfg;
    int K = c.n_members, F = c.feature_dim, C = c.y_dim, M = B * mc, maxM = c.max_rows, NT = step_partials(h, M);
    // descriptor rows by value while they fit (nm <= ND_INLINE_DESCS), else through the device tables
    const bool inl = nm <= ND_INLINE_DESCS;
    const MemberDev* mdev = inl ? nullptr : h->members_dev + m0;
    const SkinnyDesc* t2 = h->descs_dev + (size_t)L_LIN2 * K + m0;
    const SkinnyDesc* t3 = h->descs_dev + (size_t)L_LIN3 * K + m0;
    const SkinnyDesc *s2 = inl ? nullptr : t2, *s3 = inl ? nullptr : t3;     // k_skinny's table argument
    MemberInline mi{};
    SkinnyInline i2{}, i3{};
    for (int g = 0; inl && g < nm; ++g) {
        mi.m[g] = h->members_host[m0 + g];
        i2.d[g] = h->descs_host[(size_t)L_LIN2 * K + m0 + g];
        i3.d[g] = h->descs_host[(size_t)L_LIN3 * K + m0 + g];
    }
    // a sampler plan: step i evaluates eps at timestep tau[S-1-i] (the embedding row of the head and of both blocks) and its head applies
    // coefficient row S-i to the state of step i-1; the final kernel applies row 0.  T == S (check_plan).
    const int* tau = h->plan_tau.empty() ? nullptr : h->plan_tau.data();
    if (tau) io.alphas = h->plan_coef;
    // ONE launch for the whole loop where the plan allows (csrc/nd_persist.hip; it knows consecutive timesteps only)
    h->persist_last = false;
    if (h->persist_mode && inl && !tau) {
        const PersistPlan pp = nd_persist_plan(F, M, nm, C, h->half);
        if (pp.ok) {
            if (pp.err != hipSuccess) return pp.err;
            PersistArgs pa{};
            for (int g = 0; g < nm; ++g) { pa.l2[g] = i2.d[g]; pa.l3[g] = i3.d[g]; pa.mem[g] = mi.m[g]; }
            pa.io = io;
            const char* act = getenv("ND_PERSIST_ACTIVE");                  // experiments only: run the first n members of the launch
            const char* spin = getenv("ND_PERSIST_SPIN_TICKS");             // tests only: how long a barrier wait may last (100 MHz ticks)
            const char* fake = getenv("ND_PERSIST_FAKE_RESIDENT");          // timing ablation only: results are wrong (nd_persist.hpp)
            pa.s = PersistScalars{h->persist_bar, nm, B, M, maxM, F, T, h->persist_skew_ticks, spin ? atoi(spin) : 100000000 /* 1 s */,
                                  act ? atoi(act) : nm, fake ? atoi(fake) : 0};
            nd_note_h_layout(h, m0, nm, false);
            if (h->profiling && !grow_probe_events(h, 4)) return hipErrorOutOfMemory;
            hipEvent_t* ev = h->profiling ? h->probe_events.data() : nullptr;
            if (ev) em.record(ev[0]);
            void* ap[] = {&pa};
            em.emit(pp.fn, pp.grid, pp.block, ap, pp.lds);
            if (ev) em.record(ev[1]);
            h->probe_steps = 0;
            h->persist_last = true;
            return em.err;
        }
    }
    SkinnyDesc d0{};
    const dim3 ghead((F + 1023) / 1024, M, nm);
    const SkinnyLaunch L2 = nd_skinny_launch<0>(F, F, M, nm, h->half), L3 = nd_skinny_launch<1>(F, F, M, nm, h->half);
    if (L2.err != hipSuccess) return L2.err;       // the kernel's dynamic-LDS attribute could not be set on this device
    if (L3.err != hipSuccess) return L3.err;
    int cps2 = L2.cps, cps3 = L3.cps;
    // more than 128 rows: the LDS-tiled kernel (+ its fixup for the k-split tail) takes the place of each k_skinny node
    CondGemmPlan tp = nd_cond_gemm_plan(F, F, M, nm, h->half);
    float* tws = h->tile_ws;
    // ... on the bf16 matrix pipe (frag32b3 operands, exact fp32 products) where the handle holds the images: the step head then
    // writes h1 as such an image (its record travels by value, so the layout is chosen per launch; the device-table path of more
    // than ND_INLINE_DESCS members keeps the f32-input MFMA kernel)
    const bool b9 = tp.use_tile && h->b9 && inl;
    nd_note_h_layout(h, m0, nm, b9);
    if (b9) {
        t2 = h->descs_dev + (size_t)L_LIN2S * K + m0;
        t3 = h->descs_dev + (size_t)L_LIN3S * K + m0;
        for (int g = 0; g < nm; ++g) { mi.m[g].h1 = (float*)h->members[m0 + g].h1s; mi.m[g].h16 = 2; }
    }
    const dim3 tgrid((unsigned)(tp.n_full + tp.rem * tp.split)), tfix((unsigned)tp.rem * (b9 ? 16 : 4));
    // ... and the head in its many-rows form (16 rows per workgroup, whole operand planes per store; same bits)
    const bool rows_head = b9 && NT <= 64 && !getenv("ND_HEAD_PER_ROW");
    const dim3 ghead_rows((F + ND_HEAD_ROWS_COLS - 1) / ND_HEAD_ROWS_COLS, (M + 15) / 16, nm);
    void* const head_fn = nd_step_head_kernel(C, rows_head, tau != nullptr);
    // probes: up to 8 PAIRS of steps (i, i+1) spread over the loop (never step 0: its head is the cheap INIT form).  Records
    // around head(i), around the two blocks of step i, and behind the blocks of step i+1: the third interval is one whole unrecorded
    // step, so  (whole step) - (two blocks) = the head alone, and what a record node adds to an interval follows from the head's
    // own interval -- calibrated inside the loaded graph instead of by an empty interval (two record nodes back to back cost 6 us,
    // most of which a kernel launched behind a record node hides).
    const int want = h->profiling ? ((T - 1) / 2 < 8 ? (T - 1) / 2 : 8) : 0;
    const int stride = want > 0 ? (T - 1) / want : 0;
    hipEvent_t pending_end = nullptr;
    if (!grow_probe_events(h, 4 * (size_t)want)) return hipErrorOutOfMemory;
    int probed = 0;
    HeadArgs ha{mi, mdev, io, 0, 0, 0, 0, B, M, maxM, F, NT, T};
    for (int i = 0; i < T; ++i) {
        int t = tau ? tau[T - 1 - i] : T - 1 - i;
        ha.mode = (i == 0) ? ND_HEAD_INIT : ND_HEAD_UPDATE; ha.i_step = i; ha.t_prev = tau ? T - i : t + 1; ha.t = t;
        const bool probe = want > 0 && i >= 1 && i + 1 < T && !pending_end && probed < want && ((i - 1) % stride) == (stride - 1) / 2;
        hipEvent_t* ev = probe ? &h->probe_events[4 * probed] : nullptr;
        hipEvent_t end_of_pair = pending_end;      // this step closes the pair opened by the previous one
        pending_end = nullptr;
        if (probe) em.record(ev[0]);
        em.emit(head_fn, rows_head ? ghead_rows : ghead, dim3(256), ha.ptrs());
        if (probe) em.record(ev[1]);
        if (tp.use_tile) {
            void* a2[] = {&d0, &t2, &M, &t, &tp.TM, &tp.TN, &tp.n_full, &tp.split, &tws};
            void* a3[] = {&d0, &t3, &M, &t, &tp.TM, &tp.TN, &tp.n_full, &tp.split, &tws};
            if (b9) {
                em.emit(nd_cond_gemm_b9_kernel(0), tgrid, dim3(512), a2, nd_cond_gemm_b9_dynlds());
                if (tp.rem > 0) em.emit(nd_cond_gemm_b9_fixup_kernel(0), tfix, dim3(64), a2);
                em.emit(nd_cond_gemm_b9_kernel(1), tgrid, dim3(512), a3, nd_cond_gemm_b9_dynlds());
                if (tp.rem > 0) em.emit(nd_cond_gemm_b9_fixup_kernel(1), tfix, dim3(64), a3);
            } else {
                em.emit(nd_cond_gemm_kernel(0), tgrid, dim3(256), a2, nd_cond_gemm_dynlds());
                if (tp.rem > 0) em.emit(nd_cond_gemm_fixup_kernel(0), tfix, dim3(64), a2);
                em.emit(nd_cond_gemm_kernel(1), tgrid, dim3(256), a3, nd_cond_gemm_dynlds());
                if (tp.rem > 0) em.emit(nd_cond_gemm_fixup_kernel(1), tfix, dim3(64), a3);
            }
        } else {
            void* a2[] = {&i2, &s2, &nm, &M, &t, &cps2};
            em.emit(L2.fn, L2.grid, L2.block, a2, L2.lds);
            void* a3[] = {&i3, &s3, &nm, &M, &t, &cps3};
            em.emit(L3.fn, L3.grid, L3.block, a3, L3.lds);
        }
        // the two ConditionalLinear launches share ONE interval (one record node for two kernels: half the distortion per launch)
        if (probe) { em.record(ev[2]); pending_end = ev[3]; ++probed; }
        if (end_of_pair) em.record(end_of_pair);
    }
    h->probe_steps = probed;
    FinalArgs fa{mi, mdev, io, 0, (T - 1) & 1, B, M, maxM, NT, T, nullptr, 0};
    em.emit(nd_step_final_kernel(C, tau != nullptr), dim3(M, 1, nm), dim3(64), fa.ptrs());
    return em.err;
}

// The kernels of one sampling call through `em`: [Philox fill] -> 3T+1 step kernels -> [advance the batch counter].  draw: the noise
// comes from the library's counter-based generator (nd_seed), written to the workspace by the first kernel and consumed from there.
static hipError_t emit_sampling(nd_handle_s* h, Emitter& em, int m0, int nm, StepIO io, bool draw, int B, int mc, int T) {
    if (draw) {
        float* out = h->noise_ws;
        const unsigned long long* state = h->rng_state;
        unsigned long long seed0 = 0;
        uint32_t z0 = 0, z1 = 0;
        int C = h->cfg.y_dim;
        void* a[] = {&out, &state, &seed0, &z0, &z1, &m0, &nm, &T, &B, &mc, &C};
        em.emit(nd_philox_normal_kernel(), nd_philox_normal_grid(nm, T, B, mc, C), dim3(256), a);
    }
    hipError_t e = emit_loop(h, em, m0, nm, io, B, mc, T);
    if (e == hipSuccess && draw) {
        unsigned long long* state = h->rng_state;
        void* a[] = {&state};
        em.emit(nd_rng_advance_kernel(), dim3(1), dim3(64), a);
        e = em.err;
    }
    return e;
}

// ... enqueued on a stream (eager, or under the stream capture of nd_predict_batch)
static int run_loop_eager(nd_handle_s* h, hipStream_t st, int m0, int nm, StepIO io, bool draw, int B, int mc, int T) {
    Emitter em{st};
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    HIP_CHECK(hipStreamIsCapturing(st, &cs));
    em.capturing = cs == hipStreamCaptureStatusActive;
    hipError_t e = emit_sampling(h, em, m0, nm, io, draw, B, mc, T);
    if (e != hipSuccess) return nd_set_err(ND_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    return ND_OK;
}

extern "C" int nd_sample(nd_handle h, int m0, int nm, const float* yhat_dev, const float* ymean_dev, const float* noise_dev,
                         float* y0_out_dev, float* seq_out_dev, int B, int mc, int T, int use_graph, void* stream) {
    int rc = nd_check_range(h, m0, nm);
    if (rc != ND_OK) return rc;
    if (!yhat_dev || !ymean_dev || !y0_out_dev) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    rc = check_rows(h, B, mc, T);
    if (rc == ND_OK) rc = check_plan(h, T);
    if (rc != ND_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int C = h->cfg.y_dim, M = B * mc;
    const bool draw = noise_dev == nullptr;
    StepIO io{};
    io.yhat = yhat_dev;   io.yhat_ms = (size_t)B * C;
    io.ymean = ymean_dev; io.ymean_ms = (size_t)B * C;
    io.noise = draw ? h->noise_ws : noise_dev; io.noise_ms = (size_t)T * M * C;
    io.y0_out = y0_out_dev; io.y0_ms = (size_t)M * C;
    io.seq_out = seq_out_dev; io.seq_ms = (size_t)(T + 1) * M * C;
    io.alphas = h->alphas; io.omabs = h->omabs;
    if (!use_graph) return run_loop_eager(h, st, m0, nm, io, draw, B, mc, T);
    GraphKey key{m0, nm, B, mc, T, yhat_dev, ymean_dev, noise_dev, y0_out_dev, seq_out_dev};
    auto it = h->graphs.find(key);
    if (it == h->graphs.end()) {
        Emitter em{st};
        HIP_CHECK(hipGraphCreate(&em.graph, 0));
        hipError_t e = emit_sampling(h, em, m0, nm, io, draw, B, mc, T);
        if (e != hipSuccess) {
            (void)hipGraphDestroy(em.graph);
            return nd_set_err(ND_ERR_HIP, "graph build failed: %s", hipGetErrorString(e));
        }
        h->probe_nodes = count_event_record_nodes(em.graph);
        hipGraphExec_t exec;
        e = hipGraphInstantiate(&exec, em.graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(em.graph);
        if (e != hipSuccess) return nd_set_err(ND_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e));
        if (h->graphs.size() >= 64) nd_drop_graphs(h);
        it = h->graphs.emplace(key, exec).first;
    }
    HIP_CHECK(hipGraphLaunch(it->second, st));
    nd_note_h_layout(h, m0, nm, loop_writes_split(h, M, nm));
    return ND_OK;
}

// ---------------------------------------------------------------------------------------------
// The whole hot path of one test batch (classification_train_separately.py:749-794) as one call / one hipGraph:
//   :753      compute_guiding_prediction           nd_guiding_prediction (ViT prefix + mapping MLPs + softmax, :755-758)
//   :747      images_224_flat                      the same buffer viewed [B, D]
//   (hoist)   xe = norm(encoder_x(x)) per member   nd_encode, once per (member, batch) instead of once per step
//   :767-777  K members x mc trials p_sample_loop  the 3T+1 step kernels (all members and trials per launch)
//   :786-789  vote, compute_ensemble_confidence    nd_aggregate
// The graph is recorded by stream capture on a private stream (the caller's stream may be the legacy default stream, which
// cannot be captured) after one eager pass, which also makes every lazily set function attribute (dynamic LDS sizes) exist
// before the capture; it is then replayed on the caller's stream.
// ---------------------------------------------------------------------------------------------
static int batch_enqueue(nd_handle_s* h, nd_cond c, const float* images, const float* noise, const nd_batch_out* out, int B, int mc,
                         int T, float temperature, hipStream_t st) {
    const int K = h->cfg.n_members, C = h->cfg.y_dim, M = B * mc;
    const bool draw = noise == nullptr;
    int rc = nd_guiding_prediction_first(c, images, h->logits_ws, out->yhat, B, K, st);     // member k <- mapping MLP k, k < K
    if (rc != ND_OK) return rc;
    rc = encode_impl(h, 0, K, images, B, st, true);       // (the conditioner's im2col ran before: the pack here is the last reader of `images`)
    if (rc != ND_OK) return rc;
    StepIO io{};
    io.yhat = out->yhat;  io.yhat_ms = (size_t)B * C;
    io.ymean = out->yhat; io.ymean_ms = (size_t)B * C;           // y_T_mean = y_0_hat (:762, quirk Q2)
    io.noise = draw ? h->noise_ws : noise; io.noise_ms = (size_t)T * M * C;
    io.y0_out = out->samples; io.y0_ms = (size_t)M * C;          // [K][mc*B][C] == [K*mc][B][C]: member-major, then trial
    io.alphas = h->alphas; io.omabs = h->omabs;
    rc = run_loop_eager(h, st, 0, K, io, draw, B, mc, T);
    if (rc != ND_OK) return rc;
    return nd_aggregate(out->samples, out->prob, out->vote, out->probs, K * mc, B, C, temperature, st);
}

extern "C" int nd_predict_batch(nd_handle h, nd_cond c, const float* images_dev, const float* noise_dev, const nd_batch_out* out,
                                int B, int mc, int T, float temperature, int use_graph, void* stream) {
    if (!h || !h->ws) return nd_set_err(ND_ERR_STATE, "workspace not bound");
    if (!c) return nd_set_err(ND_ERR_ARG, "conditioner is NULL");
    if (!images_dev || !out || !out->samples || !out->prob || !out->vote || !out->yhat) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    const nd_cond_config* cc = nd_cond_get_config(c);
    const nd_config& g = h->cfg;
    if (cc->n_mlps < g.n_members) return nd_set_err(ND_ERR_ARG, "conditioner has %d mapping MLPs, ensemble %d members", cc->n_mlps, g.n_members);
    if (cc->num_classes != g.y_dim) return nd_set_err(ND_ERR_ARG, "conditioner has %d classes, ensemble %d", cc->num_classes, g.y_dim);
    if ((long)cc->in_chans * cc->img_size * cc->img_size != g.data_dim)
        return nd_set_err(ND_ERR_ARG, "image size %dx%dx%d != data_dim %d", cc->in_chans, cc->img_size, cc->img_size, g.data_dim);
    int rc = nd_check_range(h, 0, g.n_members);
    if (rc != ND_OK) return rc;
    if (B < 1 || B > g.max_batch || B > cc->max_batch) return nd_set_err(ND_ERR_ARG, "B=%d outside [1,%d]", B, g.max_batch < cc->max_batch ? g.max_batch : cc->max_batch);
    rc = check_rows(h, B, mc, T, false);      // the batch encodes for itself
    if (rc == ND_OK) rc = check_plan(h, T);
    if (rc != ND_OK) return rc;
    if (!(temperature > 0.f)) return nd_set_err(ND_ERR_ARG, "temperature must be > 0");
    hipStream_t st = (hipStream_t)stream;
    if (!use_graph) return batch_enqueue(h, c, images_dev, noise_dev, out, B, mc, T, temperature, st);
    unsigned tb;
    memcpy(&tb, &temperature, sizeof tb);
    BatchKey key{nd_cond_serial(c), images_dev, noise_dev, out->samples, out->prob, out->vote, out->probs, out->yhat, B, mc, T, tb, h->profiling};
    auto it = h->batch_graphs.find(key);
    if (it == h->batch_graphs.end()) {
        // first call of this shape: one eager pass on the caller's stream IS this call's result; the graph recorded next to it is
        // for the following calls
        rc = batch_enqueue(h, c, images_dev, noise_dev, out, B, mc, T, temperature, st);
        if (rc != ND_OK) return rc;
        if (!h->capture_stream) HIP_CHECK(hipStreamCreateWithFlags(&h->capture_stream, hipStreamNonBlocking));
        HIP_CHECK(hipStreamBeginCapture(h->capture_stream, hipStreamCaptureModeRelaxed));
        rc = batch_enqueue(h, c, images_dev, noise_dev, out, B, mc, T, temperature, h->capture_stream);
        hipGraph_t graph = nullptr;
        hipError_t e = hipStreamEndCapture(h->capture_stream, &graph);
        if (rc != ND_OK) {
            if (graph) (void)hipGraphDestroy(graph);
            return rc;
        }
        if (e != hipSuccess) return nd_set_err(ND_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
        h->probe_nodes = count_event_record_nodes(graph);
        hipGraphExec_t exec;
        e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) return nd_set_err(ND_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e));
        if (h->batch_graphs.size() >= 16) nd_drop_graphs(h);
        h->batch_graphs.emplace(key, exec);
        h->encoded_B = B;
        return ND_OK;
    }
    HIP_CHECK(hipGraphLaunch(it->second, st));
    nd_note_h_layout(h, 0, g.n_members, loop_writes_split(h, B * mc, g.n_members));
    h->encoded_B = B;
    return ND_OK;
}
