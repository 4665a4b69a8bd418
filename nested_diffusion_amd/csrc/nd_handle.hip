// nd_handle.hip -- the ensemble handle: workspace carving, BN/gain folding and weight packing at load time, and the small entry
// points that set or read its state.  What runs on it: csrc/nd_sampler.hip.  gfx950 only.
//
// Reference path (file:line relative to the reference checkout): diffusion/latent_model.py:93-105,169-184 (what a member holds).
#include "nd_handle.hpp"
#include "nd_cond_gemm.hpp"
#include "nd_b9.hpp"
#include "nd_persist.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>

// ---- one-time folds, computed in fp64 and rounded once --------------------------
// eval BatchNorm1d: BN(u) = s*u + o, s = w / sqrt(var + 1e-5), o = beta - mean*s
// Linear bias folded: BN(W h + b) = s*(W h) + (s*b + o)
__global__ void k_fold_bn(float* scale, float* shift, const float* lin_b, const float* bn_w, const float* bn_b,
                          const float* bn_mean, const float* bn_var, int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const double s = (double)bn_w[n] / sqrt((double)bn_var[n] + 1e-5);
    const double o = (double)bn_b[n] - (double)bn_mean[n] * s;
    scale[n] = (float)s;
    shift[n] = (float)(s * (double)lin_b[n] + o);
}
// ConditionalLinear + BN: BN(g_t * (W h + b)) = (s g_t) * (W h) + (s g_t b + o)
__global__ void k_fold_steps(float* A, float* Cc, const float* emb, const float* lin_b, const float* bn_w, const float* bn_b,
                             const float* bn_mean, const float* bn_var, int T, int N) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)T * N) return;
    const int n = (int)(i % N);
    const double s = (double)bn_w[n] / sqrt((double)bn_var[n] + 1e-5);
    const double o = (double)bn_b[n] - (double)bn_mean[n] * s;
    const double g = (double)emb[i];
    A[i] = (float)(s * g);
    Cc[i] = (float)(s * g * (double)lin_b[n] + o);
}

static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Carver {
    char* base; size_t off = 0;
    template <typename T> T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off = al256(off + count * sizeof(T));
        return p;
    }
};

static void carve(nd_handle_s* h, char* base, size_t* total) {
    const nd_config& c = h->cfg;
    const size_t K = c.n_members, H = c.hidden_dim, F = c.feature_dim, T = c.n_steps, C = c.y_dim, D = c.data_dim;
    const size_t mB = c.max_batch, mM = c.max_rows;
    const size_t pB = ((mB + 15) / 16) * 16, pM = ((mM + 15) / 16) * 16;   // rows padded to whole 16-row tiles
    h->NT = (int)((F + 15) / 16);
    h->half = c.operand_dtype == ND_DTYPE_F16;
    const size_t wdiv = h->half ? 2 : 1;                                     // packed weights: floats -> halfs
    h->enc_splitk = nd_use_splitk(c.data_dim);
    h->S0 = h->enc_splitk ? nd_skinny_launch<2>(c.data_dim, c.hidden_dim, c.max_batch, 1, h->half).S : 0;
    Carver cv{base};
    h->members_dev = cv.take<MemberDev>(K);
    h->descs_dev = cv.take<SkinnyDesc>(L_COUNT * K);
    h->spk_dev = cv.take<SkinnyDesc>(K);
    h->spke_dev = cv.take<SplitKEpiDesc>(K);
    h->alphas = cv.take<float>(T);
    h->omabs = cv.take<float>(T);
    h->rng_state = cv.take<unsigned long long>(2);
    h->persist_bar = cv.take<unsigned>(ND_PERSIST_BAR_WORDS);
    h->input_seq = cv.take<unsigned>(1);
    h->noise_ws = cv.take<float>(K * T * mM * C);
    h->logits_ws = cv.take<float>(K * mB * C);
    h->xpack = cv.take<float>(pB * D);
    h->tile_ws = cv.take<float>(nd_cond_gemm_wanted((int)mM, h->half) ? (size_t)CG_MAX_SLABS * CG_T * CG_T : 1);
    // more than 128 rows per member and fp32: the step blocks are MFMA-bound GEMMs; they run on the bf16 matrix pipe with exact
    // fp32 products when the depth allows (F % 32 == 0), which takes a frag32b3 copy of lin2 / lin3 (1.5 x their fp32 size)
    h->b9 = nd_cond_gemm_wanted((int)mM, h->half) && (F % 32) == 0 && !getenv("ND_STEP_F32_MFMA");
    for (size_t k = 0; k < K; ++k) {
        MemberHost& m = h->members[k];
        m.sc0 = cv.take<float>(H); m.sh0 = cv.take<float>(H);
        m.sc1 = cv.take<float>(H); m.sh1 = cv.take<float>(H);
        m.sc2 = cv.take<float>(F); m.sh2 = cv.take<float>(F);
        for (int l = 0; l < 3; ++l) { m.A[l] = cv.take<float>(T * F); m.Cc[l] = cv.take<float>(T * F); }
        m.w_enc0 = cv.take<float>(H * D / wdiv); m.w_enc3 = cv.take<float>(H * H / wdiv); m.w_enc6 = cv.take<float>(F * H / wdiv);
        m.w_lin2 = cv.take<float>(F * F / wdiv); m.w_lin3 = cv.take<float>(F * F / wdiv);
        m.w_lin1 = cv.take<float>(F * 2 * C); m.w_lin4 = cv.take<float>(C * F); m.b_lin4 = cv.take<float>(C);
        m.e0 = cv.take<float>(pB * H); m.e1 = cv.take<float>(pB * H); m.xe = cv.take<float>(pB * F);
        m.ybuf = cv.take<float>(2 * mM * C);
        m.h1 = cv.take<float>(pM * F); m.h2 = cv.take<float>(pM * F);
        if (h->b9) {
            m.w_lin2s = cv.take<char>(nd_b9_bytes((int)F, (int)F)); m.w_lin3s = cv.take<char>(nd_b9_bytes((int)F, (int)F));
            m.h1s = cv.take<char>(nd_b9_bytes((int)pM, (int)F)); m.h2s = cv.take<char>(nd_b9_bytes((int)pM, (int)F));
        }
        // eps partials per (row, class): F/16 from k_skinny, 2 per 128-column tile from k_cond_gemm (more than F/16 when F = 16)
        const size_t ntl_max = nd_cond_gemm_wanted((int)mM, h->half) ? (size_t)nd_cond_gemm_plan((int)F, (int)F, (int)mM, 1, h->half).ntl : 0;
        m.epart = cv.take<float>(((size_t)h->NT > ntl_max ? (size_t)h->NT : ntl_max) * mM * C);
        // split-K slabs: sized for the deepest split any (B <= max_batch, member count) launch can pick
        m.splitk = cv.take<float>(h->enc_splitk ? (size_t)(D / 16 / 64 + 1) * pB * H : 1);
    }
    *total = cv.off;
}

static int check_cfg(const nd_config* c) {
    if (!c) return nd_set_err(ND_ERR_ARG, "cfg is NULL");
    if (c->y_dim < 1 || c->y_dim > ND_MAX_C) return nd_set_err(ND_ERR_ARG, "y_dim must be in [1,%d]", ND_MAX_C);
    if (c->data_dim < 16 || c->data_dim % 16) return nd_set_err(ND_ERR_ARG, "data_dim must be a positive multiple of 16");
    if (c->hidden_dim < 16 || c->hidden_dim % 16) return nd_set_err(ND_ERR_ARG, "hidden_dim must be a positive multiple of 16");
    if (c->feature_dim < 16 || c->feature_dim % 16) return nd_set_err(ND_ERR_ARG, "feature_dim must be a positive multiple of 16");
    if (c->n_steps < 1) return nd_set_err(ND_ERR_ARG, "n_steps must be >= 1");
    if (c->operand_dtype != ND_DTYPE_F32 && c->operand_dtype != ND_DTYPE_F16)
        return nd_set_err(ND_ERR_ARG, "operand_dtype must be ND_DTYPE_F32 or ND_DTYPE_F16");
    if (c->operand_dtype == ND_DTYPE_F16 && ((c->data_dim | c->hidden_dim | c->feature_dim) % 32))
        return nd_set_err(ND_ERR_ARG, "fp16 operands need data_dim, hidden_dim and feature_dim to be multiples of 32");
    if (c->n_members < 1 || c->n_members > 255 || c->max_batch < 1 || c->max_rows < c->max_batch)
        return nd_set_err(ND_ERR_ARG, "n_members (1..255) / max_batch / max_rows invalid");
    return ND_OK;
}

extern "C" size_t nd_workspace_bytes(const nd_config* cfg) {
    if (check_cfg(cfg) != ND_OK) return 0;
    nd_handle_s tmp;
    tmp.cfg = *cfg;
    tmp.members.resize(cfg->n_members);
    size_t total = 0;
    carve(&tmp, nullptr, &total);
    return total;
}

extern "C" int nd_create(const nd_config* cfg, nd_handle* out) {
    if (!out) return nd_set_err(ND_ERR_ARG, "out is NULL");
    int rc = check_cfg(cfg);
    if (rc != ND_OK) return rc;
    nd_handle_s* h = new nd_handle_s();
    h->cfg = *cfg;
    h->members.resize(cfg->n_members);
    if (const char* e = getenv("ND_PERSIST")) h->persist_mode = atoi(e);
    if (const char* e = getenv("ND_PERSIST_SKEW_US")) h->persist_skew_ticks = (int)(atof(e) * 100.0);
    *out = h;
    return ND_OK;
}

void nd_drop_graphs(nd_handle_s* h) {
    for (auto& kv : h->graphs) (void)hipGraphExecDestroy(kv.second);
    h->graphs.clear();
    for (auto& kv : h->batch_graphs) (void)hipGraphExecDestroy(kv.second);
    h->batch_graphs.clear();
}

extern "C" int nd_destroy(nd_handle h) {
    if (!h) return ND_OK;
    nd_drop_graphs(h);
    for (hipEvent_t e : h->probe_events) (void)hipEventDestroy(e);
    if (h->capture_stream) (void)hipStreamDestroy(h->capture_stream);
    if (h->plan_coef) (void)hipFree(h->plan_coef);
    delete h;
    return ND_OK;
}

extern "C" int nd_bind_workspace(nd_handle h, void* ws, size_t bytes) {
    if (!h || !ws) return nd_set_err(ND_ERR_ARG, "handle/workspace is NULL");
    if ((uintptr_t)ws & 255) return nd_set_err(ND_ERR_ARG, "workspace must be 256-byte aligned");
    size_t need = 0;
    carve(h, (char*)ws, &need);
    if (bytes < need) return nd_set_err(ND_ERR_ARG, "workspace too small: %zu < %zu", bytes, need);
    h->ws = (char*)ws;
    h->ws_bytes = bytes;
    nd_drop_graphs(h);
    for (auto& m : h->members) m.loaded = false;
    // activations: padded tile rows must hold finite values before the first kernel reads them
    HIP_CHECK(hipMemset(h->xpack, 0, (size_t)((char*)h->members[0].sc0 - (char*)h->xpack)));
    for (auto& m : h->members) HIP_CHECK(hipMemset(m.e0, 0, (size_t)((char*)m.splitk - (char*)m.e0)));
    HIP_CHECK(hipMemset(h->rng_state, 0, 2 * sizeof(unsigned long long)));
    HIP_CHECK(hipMemset(h->persist_bar, 0, ND_PERSIST_BAR_WORDS * sizeof(unsigned)));
    HIP_CHECK(hipMemset(h->input_seq, 0, sizeof(unsigned)));
    return ND_OK;
}

extern "C" int nd_seed(nd_handle h, uint64_t seed, uint32_t first_image) {
    if (!h || !h->ws) return nd_set_err(ND_ERR_STATE, "workspace not bound");
    const unsigned long long st[2] = {(unsigned long long)seed, (unsigned long long)first_image << 32};   // batch counter 0
    HIP_CHECK(hipDeviceSynchronize());          // no sampling graph may be reading the state while it is replaced
    HIP_CHECK(hipMemcpy(h->rng_state, st, sizeof st, hipMemcpyHostToDevice));
    return ND_OK;
}

extern "C" int nd_rng_state(nd_handle h, uint64_t out[2]) {
    if (!h || !out) return nd_set_err(ND_ERR_ARG, "handle/out is NULL");
    if (!h->ws) return nd_set_err(ND_ERR_STATE, "workspace not bound");
    unsigned long long st[2];
    HIP_CHECK(hipDeviceSynchronize());          // every enqueued sampling loop has advanced the batch counter
    HIP_CHECK(hipMemcpy(st, h->rng_state, sizeof st, hipMemcpyDeviceToHost));
    out[0] = (uint64_t)st[0];
    out[1] = (uint64_t)st[1];
    return ND_OK;
}

extern "C" int nd_set_rng_state(nd_handle h, const uint64_t in[2]) {
    if (!h || !in) return nd_set_err(ND_ERR_ARG, "handle/in is NULL");
    if (!h->ws) return nd_set_err(ND_ERR_STATE, "workspace not bound");
    const unsigned long long st[2] = {(unsigned long long)in[0], (unsigned long long)in[1]};
    HIP_CHECK(hipDeviceSynchronize());          // as nd_seed: no sampling graph may be reading the state while it is replaced
    HIP_CHECK(hipMemcpy(h->rng_state, st, sizeof st, hipMemcpyHostToDevice));
    return ND_OK;
}

extern "C" int nd_set_schedule(nd_handle h, const float* alphas_dev, const float* omabs_dev, int T, void* stream) {
    if (!h || !h->ws) return nd_set_err(ND_ERR_STATE, "workspace not bound");
    if (!alphas_dev || !omabs_dev) return nd_set_err(ND_ERR_ARG, "NULL schedule");
    if (T < 1 || T > h->cfg.n_steps) return nd_set_err(ND_ERR_ARG, "T=%d outside [1,%d]", T, h->cfg.n_steps);
    hipStream_t st = (hipStream_t)stream;
    HIP_CHECK(hipMemcpyAsync(h->alphas, alphas_dev, sizeof(float) * T, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemcpyAsync(h->omabs, omabs_dev, sizeof(float) * T, hipMemcpyDeviceToDevice, st));
    h->sched_T = T;
    return ND_OK;
}

extern "C" int nd_set_sampler(nd_handle h, const int32_t* timesteps_host, const float* coef_host, int S, void* stream) {
    // every argument first: nothing is allocated, copied or dropped by a refused call
    if (!h) return nd_set_err(ND_ERR_ARG, "set_sampler: handle is NULL");
    if (S < 0 || S > h->cfg.n_steps) return nd_set_err(ND_ERR_ARG, "set_sampler: S=%d outside [0,%d]", S, h->cfg.n_steps);
    if (S > 0 && (!timesteps_host || !coef_host)) return nd_set_err(ND_ERR_ARG, "set_sampler: timesteps_host / coef_host is NULL");
    for (int j = 0; j < S; ++j) {
        const int t = timesteps_host[j];
        if (t < 0 || t >= h->cfg.n_steps) return nd_set_err(ND_ERR_ARG, "set_sampler: timesteps[%d]=%d outside [0,%d)", j, t, h->cfg.n_steps);
        if (j > 0 && t <= timesteps_host[j - 1])
            return nd_set_err(ND_ERR_ARG, "set_sampler: timesteps must be strictly increasing (timesteps[%d]=%d after %d)", j, t, timesteps_host[j - 1]);
    }
    for (int j = 0; j < 4 * S; ++j)
        if (!std::isfinite(coef_host[j])) return nd_set_err(ND_ERR_ARG, "set_sampler: coefficient [%d][%d] is not finite", j / 4, j % 4);
    if (S == 0) {
        h->plan_tau.clear();
        nd_drop_graphs(h);
        return ND_OK;
    }
    hipStream_t st = (hipStream_t)stream;
    if (h->plan_cap < S) {       // set time only: the buffer grows to the longest plan the handle has seen
        HIP_CHECK(hipDeviceSynchronize());       // no loop of an earlier plan may still be reading the buffer that is released
        if (h->plan_coef) HIP_CHECK(hipFree(h->plan_coef));
        h->plan_coef = nullptr; h->plan_cap = 0; h->plan_tau.clear();
        HIP_CHECK(hipMalloc((void**)&h->plan_coef, sizeof(float) * 4 * (size_t)S));
        h->plan_cap = S;
    }
    // behind everything enqueued on `stream` so far; the host waits, so the caller's arrays are free when this returns
    HIP_CHECK(hipMemcpyAsync(h->plan_coef, coef_host, sizeof(float) * 4 * (size_t)S, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    h->plan_tau.assign(timesteps_host, timesteps_host + S);
    nd_drop_graphs(h);
    return ND_OK;
}

extern "C" int nd_sampler_steps(nd_handle h) { return h ? (int)h->plan_tau.size() : 0; }

extern "C" int nd_load_member(nd_handle h, int k, const nd_member_weights* w, void* stream) {
    if (!h || !h->ws) return nd_set_err(ND_ERR_STATE, "workspace not bound");
    if (k < 0 || k >= h->cfg.n_members) return nd_set_err(ND_ERR_ARG, "member %d out of range", k);
    if (!w) return nd_set_err(ND_ERR_ARG, "weights is NULL");
    const void* const* pp = reinterpret_cast<const void* const*>(w);
    for (size_t i = 0; i < sizeof(nd_member_weights) / sizeof(void*); ++i)
        if (!pp[i]) return nd_set_err(ND_ERR_ARG, "nd_member_weights pointer #%zu is NULL", i);
    hipStream_t st = (hipStream_t)stream;
    const nd_config& c = h->cfg;
    const int H = c.hidden_dim, F = c.feature_dim, T = c.n_steps, C = c.y_dim, D = c.data_dim;
    MemberHost& m = h->members[k];
    auto g1 = [](int n) { return dim3((n + 255) / 256); };
    hipLaunchKernelGGL(k_fold_bn, g1(H), dim3(256), 0, st, m.sc0, m.sh0, w->enc0_b, w->bn0_w, w->bn0_b, w->bn0_mean, w->bn0_var, H);
    hipLaunchKernelGGL(k_fold_bn, g1(H), dim3(256), 0, st, m.sc1, m.sh1, w->enc3_b, w->bn1_w, w->bn1_b, w->bn1_mean, w->bn1_var, H);
    hipLaunchKernelGGL(k_fold_bn, g1(F), dim3(256), 0, st, m.sc2, m.sh2, w->enc6_b, w->norm_w, w->norm_b, w->norm_mean, w->norm_var, F);
    const float* embs[3] = {w->emb1, w->emb2, w->emb3};
    const float* lb[3] = {w->lin1_b, w->lin2_b, w->lin3_b};
    const float* bw[3] = {w->un1_w, w->un2_w, w->un3_w};
    const float* bb[3] = {w->un1_b, w->un2_b, w->un3_b};
    const float* bm[3] = {w->un1_mean, w->un2_mean, w->un3_mean};
    const float* bv[3] = {w->un1_var, w->un2_var, w->un3_var};
    const size_t tot = (size_t)T * F;
    for (int l = 0; l < 3; ++l)
        hipLaunchKernelGGL(k_fold_steps, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, m.A[l], m.Cc[l], embs[l], lb[l],
                           bw[l], bb[l], bm[l], bv[l], T, F);
    // weights -> frag16 in the workspace; the raw tensors are not referenced after this call returns
    nd_launch_pack(w->enc0_w, m.w_enc0, H, D, h->half, st);
    nd_launch_pack(w->enc3_w, m.w_enc3, H, H, h->half, st);
    nd_launch_pack(w->enc6_w, m.w_enc6, F, H, h->half, st);
    nd_launch_pack(w->lin2_w, m.w_lin2, F, F, h->half, st);
    nd_launch_pack(w->lin3_w, m.w_lin3, F, F, h->half, st);
    if (h->b9) {
        int rc = nd_split_rows(w->lin2_w, m.w_lin2s, F, F, st);
        if (rc == ND_OK) rc = nd_split_rows(w->lin3_w, m.w_lin3s, F, F, st);
        if (rc != ND_OK) return rc;
        HIP_CHECK(nd_cond_gemm_b9_prepare());
    }
    HIP_CHECK(hipMemcpyAsync(m.w_lin1, w->lin1_w, sizeof(float) * F * 2 * C, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemcpyAsync(m.w_lin4, w->lin4_w, sizeof(float) * C * F, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemcpyAsync(m.b_lin4, w->lin4_b, sizeof(float) * C, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipGetLastError());

    MemberDev md{m.w_lin1, m.b_lin4, m.A[0], m.Cc[0], m.xe, m.h1, m.ybuf, m.epart, h->half};
    const int opk = h->half ? 2 : 1;     // layout of an activation that feeds the next GEMM
    SkinnyDesc ds[L_COUNT];
    ds[L_ENC0] = SkinnyDesc{h->xpack, m.w_enc0, m.sc0, m.sh0, m.e0, nullptr, nullptr, D, H, C, ND_ACT_SOFTPLUS, opk};
    ds[L_ENC1] = SkinnyDesc{m.e0, m.w_enc3, m.sc1, m.sh1, m.e1, nullptr, nullptr, H, H, C, ND_ACT_SOFTPLUS, opk};
    ds[L_ENC2] = SkinnyDesc{m.e1, m.w_enc6, m.sc2, m.sh2, m.xe, nullptr, nullptr, H, F, C, ND_ACT_NONE, 1};
    ds[L_LIN2] = SkinnyDesc{m.h1, m.w_lin2, m.A[1], m.Cc[1], m.h2, nullptr, nullptr, F, F, C, ND_ACT_SOFTPLUS, opk};
    ds[L_LIN3] = SkinnyDesc{m.h2, m.w_lin3, m.A[2], m.Cc[2], nullptr, m.w_lin4, m.epart, F, F, C, ND_ACT_SOFTPLUS, 0};
    // each block's stream ends by touching the first lines of the next launch's stream (SkinnyDesc::pf): lin2 -> lin3 of the same step,
    // lin3 -> lin2 of the next one.  ND_NO_XPREFETCH=1: off (the A/B switch).
    if (!getenv("ND_NO_XPREFETCH")) { ds[L_LIN2].pf = m.w_lin3; ds[L_LIN3].pf = m.w_lin2; }
    ds[L_LIN2S] = ds[L_LIN2]; ds[L_LIN3S] = ds[L_LIN3];
    if (h->b9) {   // the same two blocks on frag32b3 operands: h1s -> lin2 -> h2s (out_packed 3) -> lin3 + lin4 -> eps partials
        ds[L_LIN2S].x = (const float*)m.h1s; ds[L_LIN2S].w = (const float*)m.w_lin2s; ds[L_LIN2S].out = (float*)m.h2s; ds[L_LIN2S].out_packed = 3;
        ds[L_LIN3S].x = (const float*)m.h2s; ds[L_LIN3S].w = (const float*)m.w_lin3s;
    }
    {
        // INFINITY-CACHE RESIDENCY.  A step streams 2 K F^2 weights (671 MB at K = 5, fp32), far more than the 256 MiB Infinity
        // Cache, so the step kernels read W with nontemporal loads -- nothing survives to the next step.  Reading the first
        // ND_KEEP_BYTES of them (lin2 of member 0, 1, .. then lin3) with default-policy loads instead keeps exactly those resident
        // from step to step while the nontemporal rest streams past them.  Measured (K = 5, T = 100, B = 32; sampler ms):
        //   fp32: none 13.43 | 1+1 matrices 12.57 | 3+0 12.36 | 4+0 12.58 | 3+1 12.63 | all 14.44      (a matrix = 67 MB)
        //   fp16: none  7.67 | 5+0 7.11 | 5+1 6.88 | 5+2 6.96 | all 7.91                                 (a matrix = 34 MB)
        // i.e. ~200 MB is what stays (the rest of the cache turns over with activations, tables and the streamed lines).
        const double mat = (double)F * F * (h->half ? 2.0 : 4.0);
        const char* keep_mb = getenv("ND_KEEP_MB");                       // experiments: another residency budget (MB)
        const int n_keep = (int)((keep_mb ? atof(keep_mb) * 1e6 : ND_KEEP_BYTES) / mat);
        ds[L_LIN2].keep = k < n_keep;
        ds[L_LIN3].keep = c.n_members + k < n_keep;
        if (const char* plan = getenv("ND_KEEP_PLAN")) {                  // experiments: "a,b" = lin2 of members < a, lin3 of members < b
            int a = 0, b = 0;
            if (sscanf(plan, "%d,%d", &a, &b) == 2) { ds[L_LIN2].keep = k < a; ds[L_LIN3].keep = k < b; }
        }
    }
    // small synchronous H2D copies: load time only, never on the sampling path.  The sync also means the
    // caller may release its raw weight tensors as soon as this function returns.
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipMemcpy(h->members_dev + k, &md, sizeof md, hipMemcpyHostToDevice));
    h->members_host.resize(c.n_members);
    h->descs_host.resize((size_t)L_COUNT * c.n_members);
    h->members_host[k] = md;
    for (int l = 0; l < L_COUNT; ++l) {
        h->descs_host[(size_t)l * c.n_members + k] = ds[l];
        HIP_CHECK(hipMemcpy(h->descs_dev + (size_t)l * c.n_members + k, &ds[l], sizeof(SkinnyDesc), hipMemcpyHostToDevice));
    }
    if (h->enc_splitk) {
        SkinnyDesc sd{h->xpack, m.w_enc0, nullptr, nullptr, nullptr, nullptr, m.splitk, D, H, C, ND_ACT_NONE, 0};
        SplitKEpiDesc se{m.splitk, m.sc0, m.sh0, m.e0, H, 0 /* S is a launch argument */, ND_ACT_SOFTPLUS, opk};
        HIP_CHECK(hipMemcpy(h->spk_dev + k, &sd, sizeof sd, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(h->spke_dev + k, &se, sizeof se, hipMemcpyHostToDevice));
    }
    m.loaded = true;
    nd_drop_graphs(h);
    return ND_OK;
}

int nd_check_range(nd_handle_s* h, int m0, int nm) {
    if (!h || !h->ws) return nd_set_err(ND_ERR_STATE, "workspace not bound");
    if (m0 < 0 || nm < 1 || m0 + nm > h->cfg.n_members) return nd_set_err(ND_ERR_ARG, "member range [%d,%d) invalid", m0, m0 + nm);
    for (int k = m0; k < m0 + nm; ++k)
        if (!h->members[k].loaded) return nd_set_err(ND_ERR_STATE, "member %d not loaded", k);
    return ND_OK;
}

void nd_note_h_layout(nd_handle_s* h, int m0, int nm, bool split) {
    for (int k = m0; k < m0 + nm; ++k) h->members[k].h_split = split;
}

extern "C" int nd_member_buffer(nd_handle h, int k, int which, float* dst_dev, int rows, void* stream) {
    // arguments first (host-only callers get the same answers on an unbound handle), then the state
    if (!h || !dst_dev) return nd_set_err(ND_ERR_ARG, "bad argument");
    if (k < 0 || k >= h->cfg.n_members) return nd_set_err(ND_ERR_ARG, "member out of range");
    if (which < 0 || which > 4) return nd_set_err(ND_ERR_ARG, "which=%d unknown", which);
    if (rows < 1 || rows > h->cfg.max_rows) return nd_set_err(ND_ERR_ARG, "rows out of range");
    const bool enc = which == 0 || which >= 3;       // xe, e0, e1: written by nd_encode, one row per image
    if (enc && rows > h->cfg.max_batch) return nd_set_err(ND_ERR_ARG, "%s holds at most max_batch rows", which == 0 ? "xe" : which == 3 ? "e0" : "e1");
    if (!h->ws) return nd_set_err(ND_ERR_STATE, "workspace not bound");
    MemberHost& m = h->members[k];
    const float* src = which == 0 ? m.xe : which == 1 ? m.h1 : which == 2 ? m.h2 : which == 3 ? m.e0 : m.e1;
    const int W = which >= 3 ? h->cfg.hidden_dim : h->cfg.feature_dim;      // e0 / e1 are hidden_dim wide
    // above 128 rows the step blocks of an fp32 handle run on frag32b3 images of h1 / h2 (bf16 matrix pipe): the live copies are
    // whichever the LAST launch over this member wrote (MemberHost::h_split), not what `rows` would pick
    if (!enc && m.h_split) return nd_join_rows(which == 1 ? m.h1s : m.h2s, dst_dev, rows, W, stream);
    nd_launch_unpack(src, dst_dev, rows, W, h->half && which != 0, (hipStream_t)stream);   // e0/e1/h1/h2 are GEMM operands (fp16 in that mode); xe never is
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" long long nd_resident_weight_bytes(nd_handle h, int block) {
    if (!h || block < 0 || block > 1 || h->descs_host.empty()) return -1;
    const int K = h->cfg.n_members, F = h->cfg.feature_dim;
    long long n = 0;
    for (int k = 0; k < K; ++k)
        if (h->members[k].loaded && h->descs_host[(size_t)(block ? L_LIN3 : L_LIN2) * K + k].keep) n += (long long)F * F * (h->half ? 2 : 4);
    return n;
}

extern "C" int nd_set_profiling(nd_handle h, int enable) {
    if (!h) return nd_set_err(ND_ERR_ARG, "handle is NULL");
    if (h->profiling != (enable != 0)) nd_drop_graphs(h);
    h->profiling = enable != 0;
    return ND_OK;
}

extern "C" int nd_set_input_flag(nd_handle h, uint32_t* flag_host_visible) {
    if (!h || !h->ws) return nd_set_err(ND_ERR_STATE, "workspace not bound");
    if ((uintptr_t)flag_host_visible & 3) return nd_set_err(ND_ERR_ARG, "flag must be 4-byte aligned");
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemset(h->input_seq, 0, sizeof(unsigned)));
    h->input_flag = flag_host_visible;
    nd_drop_graphs(h);
    return ND_OK;
}
