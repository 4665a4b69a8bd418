// nd_linear.hip -- the weight-streaming Linear (nd_linear; mapping/models/mlp.py:25-28), the mapping-MLP chain built on it
// (nd_linear.hpp) and the launch-plan introspection of the streaming and tiled kernels.  Host code only: the kernels are those of
// nd_skinny_m*.hip and nd_cond_gemm.hip.
#include "nd_frag.hpp"
#include "nd_skinny.hpp"
#include "nd_cond_gemm.hpp"
#include "nd_linear.hpp"

// ---- nd_linear: mapping/models/mlp.py:25-28 ---------------------------------------------------
extern "C" size_t nd_linear_workspace_bytes(int M, int K, int N, int dtype) {
    if (nd_bad_dtype(dtype) || M < 1 || K < nd_kmul(dtype) || (K % nd_kmul(dtype)) || N < 1) return 0;
    const int half = dtype == ND_DTYPE_F16;
    size_t bytes = nd_packed_bytes_dt(M, K, half) + 256;
    if (nd_use_splitk(K)) bytes += nd_splitk_part_floats(M, K, N, 1, half) * sizeof(float);
    else bytes += nd_cond_gemm_plan(K, N, M, 1, half).ws_bytes;      // k-slab accumulators of the large-M kernel's split tail
    return bytes + 256;
}

// The carve of that workspace -- align to 256, packed x, align to 256, partial sums -- and the pack of x [M][K] into its first part.
static int pack_input(const float* x, int M, int K, int dtype, void* ws, float** xpk, float** part, void* stream) {
    *xpk = (float*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    *part = (float*)((char*)*xpk + ((nd_packed_bytes_dt(M, K, dtype == ND_DTYPE_F16) + 255) & ~(size_t)255));
    return nd_pack_rows(x, *xpk, M, K, dtype, stream);
}

// One Linear on an ALREADY PACKED input: out = act(scale * (x . W^T) + shift); out_packed 0 row-major fp32, 1 frag16, 2 frag32h (the
// layout the next streaming layer reads).  part: split-K partial sums / k-slab accumulators (nd_linear_workspace_bytes minus the
// packed-x share).
static int linear_packed(const float* xpk, const float* wf, const float* scale, const float* shift, float* out, int M, int K, int N, int act,
                         int half, int out_packed, float* part, hipStream_t st) {
    if (nd_use_splitk(K)) {
        const SkinnyLaunch L = nd_skinny_launch<2>(K, N, M, 1, half);
        SkinnyDesc sd{xpk, wf, nullptr, nullptr, nullptr, nullptr, part, K, N, 0, ND_ACT_NONE, 0};
        HIP_CHECK(nd_launch_skinny(L, sd, nullptr, 1, M, 0, st));
        SplitKEpiDesc se{part, scale, shift, out, N, L.S, act, out_packed};
        nd_launch_splitk_epilogue(se, nullptr, 1, M, N, L.S, st);
    } else {
        SkinnyDesc d{xpk, wf, scale, shift, out, nullptr, nullptr, K, N, 0, act, out_packed};
        const CondGemmPlan tp = nd_cond_gemm_plan(K, N, M, 1, half);
        if (tp.use_tile) HIP_CHECK(nd_launch_cond_gemm(0, tp, d, nullptr, M, 0, part, st));      // more than 128 rows: LDS-tiled
        else HIP_CHECK(nd_launch_skinny(nd_skinny_launch<0>(K, N, M, 1, half), d, nullptr, 1, M, 0, st));
    }
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_linear(const float* x, const void* wpk, const float* scale, const float* shift, float* out, int M, int K, int N,
                         int act, int dtype, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !wpk || !out) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (nd_bad_dtype(dtype)) return nd_set_err(ND_ERR_ARG, "unknown dtype %d", dtype);
    if (M < 1 || N < 1 || K < nd_kmul(dtype) || (K % nd_kmul(dtype)))
        return nd_set_err(ND_ERR_ARG, "need M,N >= 1 and K a positive multiple of %d (K=%d)", nd_kmul(dtype), K);
    if (act < 0 || act > 3) return nd_set_err(ND_ERR_ARG, "unknown activation %d", act);
    const size_t need = nd_linear_workspace_bytes(M, K, N, dtype);
    if (!ws || ws_bytes < need) return nd_set_err(ND_ERR_ARG, "workspace too small: %zu < %zu", ws_bytes, need);
    float *xpk, *part;
    int rc = pack_input(x, M, K, dtype, ws, &xpk, &part, stream);
    if (rc != ND_OK) return rc;
    return linear_packed(xpk, (const float*)wpk, scale, shift, out, M, K, N, act, dtype == ND_DTYPE_F16, 0, part, (hipStream_t)stream);
}

// mapping/models/mlp.py:23-29 as ONE sequence on packed activations (library-internal; nd_conditioner.hip): the input is packed
// once, every hidden layer's epilogue writes its output in the fragment order the next layer streams (the same values nd_linear's
// row-major output + re-pack would give, fp16 rounding included), the last layer writes row-major logits.
//   dims[5] = {in, w1, w2, w3, classes}; hid[l]: >= 16*ceil(M/16) * dims[l+1] floats; ws: >= the largest nd_linear_workspace_bytes of
//   the four layers.
int nd_mlp_chain(const float* x, const void* const* wpk, const float* const* bias, const int* dims, float* const* hid, float* logits,
                 int M, int dtype, void* ws, size_t ws_bytes, void* stream) {
    const int half = dtype == ND_DTYPE_F16, opk = half ? 2 : 1;
    for (int l = 0; l < 4; ++l)
        if (ws_bytes < nd_linear_workspace_bytes(M, dims[l], dims[l + 1], dtype))
            return nd_set_err(ND_ERR_ARG, "mlp chain workspace too small for layer %d", l + 1);
    float *xpk, *part;
    int rc = pack_input(x, M, dims[0], dtype, ws, &xpk, &part, stream);
    if (rc != ND_OK) return rc;
    const float* in = xpk;
    for (int l = 0; l < 4; ++l) {
        float* out = l < 3 ? hid[l] : logits;
        // layers 2..4 read a packed activation of the previous epilogue; their split-K / k-slab scratch can start at the workspace base
        rc = linear_packed(in, (const float*)wpk[l], nullptr, bias[l], out, M, dims[l], dims[l + 1], l < 3 ? ND_ACT_RELU : ND_ACT_NONE, half,
                           l < 3 ? opk : 0, l == 0 ? part : xpk, (hipStream_t)stream);
        if (rc != ND_OK) return rc;
        in = out;
    }
    return ND_OK;
}

// The same Classifier.forward for SEVERAL mapping MLPs whose first layers have already run (nd_mlp_chain_first): layers 2..4 of all nm
// members as THREE launches instead of 3 * nm -- the members' weights differ, their shapes do not, so one k_skinny launch streams the
// nm weight matrices side by side exactly as a step block streams the K noise estimators' (descriptors by value).  At config dims a
// single member's layer is 33 MB / 1 MB / 1 KB of weights: launch-latency bound on its own (11 us each, 15 launches per batch).
// Values are those of the one-member launches up to the dealing of k-chunks to waves (fixed per geometry: reproducible).
// batchable: every one of the three layers is a plain streaming launch (no split-K, no LDS-tiled form) and nm fits the inline table.
bool nd_mlp_tail_batchable(const int* dims, int M, int nm, int dtype) {
    const int half = dtype == ND_DTYPE_F16;
    if (nm < 2 || nm > ND_INLINE_DESCS) return false;
    for (int l = 1; l < 4; ++l)
        if (nd_use_splitk(dims[l]) || nd_cond_gemm_plan(dims[l], dims[l + 1], M, nm, half).use_tile || nd_cond_gemm_plan(dims[l], dims[l + 1], M, 1, half).use_tile)
            return false;
    return true;
}

// layer 1 of one mapping MLP (the 150528-wide split-K stream): hid0 = relu(x W1^T + b1), written packed for layer 2
int nd_mlp_chain_first(const float* x, const void* w1pk, const float* bias1, const int* dims, float* hid0, int M, int dtype, void* ws,
                       size_t ws_bytes, void* stream) {
    const int half = dtype == ND_DTYPE_F16, opk = half ? 2 : 1;
    if (ws_bytes < nd_linear_workspace_bytes(M, dims[0], dims[1], dtype)) return nd_set_err(ND_ERR_ARG, "mlp chain workspace too small for layer 1");
    float *xpk, *part;
    int rc = pack_input(x, M, dims[0], dtype, ws, &xpk, &part, stream);
    if (rc != ND_OK) return rc;
    return linear_packed(xpk, (const float*)w1pk, nullptr, bias1, hid0, M, dims[0], dims[1], ND_ACT_RELU, half, opk, part, (hipStream_t)stream);
}

// layers 2..4 of nm members: hid[l][k] = member k's activation after layer l+1 (packed), logits + k * logits_stride = its output
int nd_mlp_chain_tail(int nm, const nd_mlp_weights* w, const int* dims, float* const* hid0, float* const* hid1, float* const* hid2, float* logits,
                      size_t logits_stride, int M, int dtype, void* stream) {
    const int half = dtype == ND_DTYPE_F16, opk = half ? 2 : 1;
    if (!nd_mlp_tail_batchable(dims, M, nm, dtype)) return nd_set_err(ND_ERR_ARG, "mlp tail of %d members at %d rows is not batchable", nm, M);
    float* const* in[3] = {hid0, hid1, hid2};
    float* const* outp[2] = {hid1, hid2};
    for (int l = 1; l < 4; ++l) {
        SkinnyDesc d[ND_INLINE_DESCS];
        for (int k = 0; k < nm; ++k)
            d[k] = SkinnyDesc{in[l - 1][k], (const float*)w[k].w_packed[l], nullptr, w[k].bias[l], l < 3 ? outp[l - 1][k] : logits + (size_t)k * logits_stride,
                              nullptr, nullptr, dims[l], dims[l + 1], 0, l < 3 ? ND_ACT_RELU : ND_ACT_NONE, l < 3 ? opk : 0, 0};
        HIP_CHECK(nd_launch_skinny_inline(nd_skinny_launch<0>(dims[l], dims[l + 1], M, nm, half), d, nm, M, 0, (hipStream_t)stream));
    }
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

// ---- launch-plan introspection (host only; no GPU needed) -------------------------------------
extern "C" int nd_skinny_plan(int K, int N, int M, int n_members, int dtype, int mode, int* out6) {
    if (!out6) return nd_set_err(ND_ERR_ARG, "out6 is NULL");
    if (nd_bad_dtype(dtype) || M < 1 || N < 1 || n_members < 1 || K < nd_kmul(dtype) || (K % nd_kmul(dtype)) || mode < 0 || mode > 2)
        return nd_set_err(ND_ERR_ARG, "bad shape / dtype / mode");
    const int half = dtype == ND_DTYPE_F16;
    const SkinnyLaunch L = mode == 0 ? nd_skinny_launch<0>(K, N, M, n_members, half)
                         : mode == 1 ? nd_skinny_launch<1>(K, N, M, n_members, half) : nd_skinny_launch<2>(K, N, M, n_members, half);
    const int nfr = (N + 15) / 16, wpm = (int)L.grid.x / n_members;
    out6[0] = (int)L.grid.x; out6[1] = (int)L.grid.y; out6[2] = (int)L.grid.z;
    out6[3] = (nfr + wpm - 1) / wpm;        // fragment slots per workgroup (the kernel's NF)
    out6[4] = L.cps;                        // k-chunks per slab
    out6[5] = (int)L.block.x;
    return ND_OK;
}

// Row fragments (16 rows each) a k_skinny workgroup keeps per pass over the weights at M rows: nd_pick_mt, the kernel's MT.
extern "C" int nd_skinny_row_fragments(int M) {
    if (M < 1) return nd_set_err(ND_ERR_ARG, "M must be >= 1");
    return nd_pick_mt(M);
}

// Which kernel a ConditionalLinear block of the sampler (K = N = F) runs at M = B*mc rows, and its tile plan.
extern "C" int nd_step_plan(int F, int M, int n_members, int dtype, int* out8) {
    if (!out8) return nd_set_err(ND_ERR_ARG, "out8 is NULL");
    if (nd_bad_dtype(dtype) || M < 1 || n_members < 1 || F < nd_kmul(dtype) || (F % nd_kmul(dtype))) return nd_set_err(ND_ERR_ARG, "bad shape / dtype");
    const CondGemmPlan p = nd_cond_gemm_plan(F, F, M, n_members, dtype == ND_DTYPE_F16);
    out8[0] = p.use_tile;                              // 0: k_skinny (weight streaming), 1: k_cond_gemm (LDS-tiled)
    out8[1] = p.n_full + p.rem * p.split;              // workgroups of the tiled launch
    out8[2] = p.n_full; out8[3] = p.rem; out8[4] = p.split;
    out8[5] = p.use_tile ? p.ntl : (F + 15) / 16;      // partial sums per (row, class) left for the step head
    out8[6] = p.TM; out8[7] = p.TN;
    return ND_OK;
}
