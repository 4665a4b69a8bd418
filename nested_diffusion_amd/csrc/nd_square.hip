// nd_square.hip -- the attack side of a Square-attack query (Andriushchenko et al., the Linf form of autoattack's square.py); the listing is
// in nested_diffusion_amd/square.py.  gfx950 only, all arithmetic fp32.
//   k_square_init      the vertical-stripe start over whole images: x_best = x_new = clip(x0 + eps * sigma(b, c, w), lo, hi)
//   k_square_propose   per active row: the window and the per-channel signs of this query drawn from Philox, the candidate written into the
//                      window of x_new, the window's corner into win
//   k_square_accept    per-image bookkeeping of one query (one thread per image): the margin, the accept rule, the flags
//   k_square_commit    per active row, over the window: an accepted candidate becomes x_best, a rejected one is restored from x_best
//
// A query is three launches around the model's forward pass: propose, (forward), accept, commit.  They are kept apart on purpose: the
// window a commit restores and the window the next propose writes overlap in the same row, and stream order between two launches is what
// keeps "restore, then perturb" in that order without a grid-wide barrier.
//
// Windows start at arbitrary (vh, vw) and W need not be a multiple of 4: every window access is a scalar fp32 load or store, consecutive
// lanes on consecutive w (coalesced along a window row); nothing assumes 16-byte alignment inside an image.  A window of side s moves
// Cin * s * s elements per image, against Cin * H * W for the whole-array formulation.
#include "nd_attack.hpp"
#include "nd_philox.hpp"

// every operation below is one rounded fp32 op in the listed order: a float32 restatement on the host reproduces every array bit for bit
#pragma clang fp contract(off)

namespace {

constexpr int SQ_THREADS = ND_ATTACK_THREADS;
constexpr int SQ_INIT_ROWS = 8;          // image rows per workgroup of the start: one Philox call serves them all
constexpr int SQ_MAX_DIM = 4096;         // H, W: Cin * s * s <= 2^29, so a window's element counter (plus one grid stride) stays inside int

// grid (ceil(Cin * W / 256), ceil(H / SQ_INIT_ROWS), B): thread j = c * W + w owns column w of channel c over the workgroup's rows
__global__ __launch_bounds__(SQ_THREADS) void k_square_init(const float* __restrict__ x0, const int64_t* __restrict__ index, float* __restrict__ x_best,
                                                            float* __restrict__ x_new, int Cin, int H, int W, uint64_t seed, uint32_t restart,
                                                            float eps, float lo, float hi) {
    const int j = blockIdx.x * SQ_THREADS + threadIdx.x;
    if (j >= Cin * W) return;
    const int b = blockIdx.z, c = j / W, w = j - c * W;
    uint32_t p[4] = {(uint32_t)index[b], (uint32_t)j >> 2, restart, ND_SQUARE_INIT_TAG};
    nd_philox4x32_10(p, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float sigma = (p[j & 3] >> 31) ? 1.0f : -1.0f;
    const float d = eps * sigma;
    const int h0 = blockIdx.y * SQ_INIT_ROWS, h1 = min(h0 + SQ_INIT_ROWS, H);
    const size_t base = ((size_t)b * Cin + c) * H * W + w;
    for (int h = h0; h < h1; ++h) {
        const size_t o = base + (size_t)h * W;
        const float v = nd_clampf(x0[o] + d, lo, hi);
        x_best[o] = v;
        x_new[o] = v;
    }
}

// grid (blocks per image, B): element e of a row's window is (c, dh, dw) = (e / s^2, (e % s^2) / s, e % s); grid-stride over Cin * s^2.
// A frozen row (margin_min > 0 is false: <= 0, -0.0 and NaN alike) returns before any write.
__global__ __launch_bounds__(SQ_THREADS) void k_square_propose(const float* __restrict__ x0, const float* __restrict__ x_best, float* __restrict__ x_new,
                                                               const int64_t* __restrict__ index, const float* __restrict__ margin_min,
                                                               int32_t* __restrict__ win, int Cin, int H, int W, int s, uint32_t iter, uint64_t seed,
                                                               uint32_t restart, float eps, float lo, float hi) {
    const int b = blockIdx.y;
    if (!(margin_min[b] > 0.0f)) return;
    uint32_t p[4] = {(uint32_t)index[b], iter, restart, ND_SQUARE_STEP_TAG};
    nd_philox4x32_10(p, (uint32_t)seed, (uint32_t)(seed >> 32));
    const int vh = (int)__umulhi(p[0], (uint32_t)(H - s + 1));        // (uint64(w0) * (H - s + 1)) >> 32: in [0, H - s]
    const int vw = (int)__umulhi(p[1], (uint32_t)(W - s + 1));
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        win[2 * b] = vh;
        win[2 * b + 1] = vw;
    }
    const float two_eps = eps + eps;
    const int ss = s * s, n = Cin * ss;
    const size_t img = (size_t)b * Cin * H * W;
    for (int e = blockIdx.x * SQ_THREADS + threadIdx.x; e < n; e += gridDim.x * SQ_THREADS) {
        const int c = e / ss, r = e - c * ss, dh = r / s, dw = r - dh * s;
        const size_t o = img + ((size_t)c * H + (vh + dh)) * W + (vw + dw);
        const float d = ((p[2] >> c) & 1u) ? two_eps : -two_eps;
        const float x = x0[o];
        x_new[o] = nd_clampf(fminf(fmaxf(x_best[o] + d, x - eps), x + eps), lo, hi);
    }
}

// one thread per image.  margin = scores[y] - max_{j != y} scores[j] (the first maximal index; ties do not change the value); any NaN
// in the row, or a label outside [0, C), makes the margin NaN, and a NaN margin neither improves nor counts as fooled.
__global__ __launch_bounds__(64) void k_square_accept(const float* __restrict__ scores, const int64_t* __restrict__ labels, float* __restrict__ margin_min,
                                                      float* __restrict__ loss_min, int32_t* __restrict__ n_queries, int32_t* __restrict__ flags, int B,
                                                      int C, int iter) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float mm = margin_min[b];
    if (iter >= 0 && !(mm > 0.0f)) {            // frozen: nothing but the flag
        flags[b] = 0;
        return;
    }
    const float* sc = scores + (size_t)b * C;
    const int64_t y = labels[b];
    float other = -INFINITY, at_label = NAN;
    bool nan = y < 0 || y >= C;
    for (int j = 0; j < C; ++j) {
        const float v = sc[j];
        nan = nan || v != v;
        if (j == y) at_label = v;
        else if (v > other) other = v;
    }
    const float margin = nan ? NAN : at_label - other;
    const float loss = margin;
    if (iter < 0) {
        margin_min[b] = margin;
        loss_min[b] = loss;
        n_queries[b] = 1;
        flags[b] = 0;
        return;
    }
    const bool improved = loss < loss_min[b];
    if (improved) loss_min[b] = loss;
    const bool accept = improved || margin <= 0.0f;
    if (accept) margin_min[b] = margin;
    n_queries[b] = n_queries[b] + 1;
    flags[b] = ND_SQUARE_ACTIVE | (accept ? ND_SQUARE_ACCEPT : 0);
}

// grid as k_square_propose.  ACTIVE | ACCEPT: x_best = x_new over the window; ACTIVE alone: x_new = x_best (the candidate is taken back);
// no ACTIVE bit: nothing.  The corner comes from device memory: one that does not keep the window inside the image is ignored.
__global__ __launch_bounds__(SQ_THREADS) void k_square_commit(float* __restrict__ x_best, float* __restrict__ x_new, const int32_t* __restrict__ win,
                                                              const int32_t* __restrict__ flags, int Cin, int H, int W, int s) {
    const int b = blockIdx.y;
    const int f = flags[b];
    if (!(f & ND_SQUARE_ACTIVE)) return;
    const int vh = win[2 * b], vw = win[2 * b + 1];
    if (vh < 0 || vw < 0 || vh > H - s || vw > W - s) return;
    const bool accept = (f & ND_SQUARE_ACCEPT) != 0;
    const int ss = s * s, n = Cin * ss;
    const size_t img = (size_t)b * Cin * H * W;
    for (int e = blockIdx.x * SQ_THREADS + threadIdx.x; e < n; e += gridDim.x * SQ_THREADS) {
        const int c = e / ss, r = e - c * ss, dh = r / s, dw = r - dh * s;
        const size_t o = img + ((size_t)c * H + (vh + dh)) * W + (vw + dw);
        if (accept) x_best[o] = x_new[o];
        else x_new[o] = x_best[o];
    }
}

// the checks every image-shaped entry point shares; 0 or the error already recorded
int sq_check_image(const char* what, int B, int Cin, int H, int W) {
    if (B < 1 || B > 65535) return nd_set_err(ND_ERR_ARG, "%s needs 1 <= B <= 65535 (B=%d)", what, B);
    if (Cin < 1 || Cin > 32) return nd_set_err(ND_ERR_ARG, "%s needs 1 <= Cin <= 32 (Cin=%d)", what, Cin);
    if (H < 1 || W < 1 || H > SQ_MAX_DIM || W > SQ_MAX_DIM)
        return nd_set_err(ND_ERR_ARG, "%s needs 1 <= H, W <= %d (H=%d, W=%d)", what, SQ_MAX_DIM, H, W);
    return ND_OK;
}

int sq_check_side(const char* what, int H, int W, int s) {
    if (s < 1 || s > H || s > W) return nd_set_err(ND_ERR_ARG, "%s needs 1 <= s <= min(H, W) (s=%d, H=%d, W=%d)", what, s, H, W);
    return ND_OK;
}

// a window's Cin * s * s elements in workgroups of 256: at most this many workgroups per image, grid-stride beyond
constexpr unsigned SQ_MAX_BLOCKS = 1024;

}  // namespace

extern "C" int nd_square_init(const float* x0, const int64_t* index, float* x_best, float* x_new, int B, int Cin, int H, int W, uint64_t seed,
                              uint32_t restart, float eps, float lo, float hi, void* stream) {
    if (!x0 || !index || !x_best || !x_new) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (int rc = sq_check_image("square init", B, Cin, H, W)) return rc;
    const dim3 grid((unsigned)((Cin * W + SQ_THREADS - 1) / SQ_THREADS), (unsigned)((H + SQ_INIT_ROWS - 1) / SQ_INIT_ROWS), (unsigned)B);
    hipLaunchKernelGGL(k_square_init, grid, dim3(SQ_THREADS), 0, (hipStream_t)stream, x0, index, x_best, x_new, Cin, H, W, seed, restart, eps, lo, hi);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_square_propose(const float* x0, const float* x_best, float* x_new, const int64_t* index, const float* margin_min, int32_t* win,
                                 int B, int Cin, int H, int W, int s, int iter, uint64_t seed, uint32_t restart, float eps, float lo, float hi,
                                 void* stream) {
    if (!x0 || !x_best || !x_new || !index || !margin_min || !win) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (int rc = sq_check_image("square propose", B, Cin, H, W)) return rc;
    if (int rc = sq_check_side("square propose", H, W, s)) return rc;
    if (iter < 0) return nd_set_err(ND_ERR_ARG, "square propose needs iter >= 0 (iter=%d)", iter);
    hipLaunchKernelGGL(k_square_propose, nd_image_grid(B, (size_t)Cin * s * s, SQ_MAX_BLOCKS), dim3(SQ_THREADS), 0, (hipStream_t)stream, x0, x_best,
                       x_new, index, margin_min, win, Cin, H, W, s, (uint32_t)iter, seed, restart, eps, lo, hi);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_square_accept(const float* scores, const int64_t* labels, float* margin_min, float* loss_min, int32_t* n_queries, int32_t* flags,
                                int B, int C, int iter, void* stream) {
    if (!scores || !labels || !margin_min || !loss_min || !n_queries || !flags) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (B < 1 || B > 65535) return nd_set_err(ND_ERR_ARG, "square accept needs 1 <= B <= 65535 (B=%d)", B);
    if (C < 2 || C > 1024) return nd_set_err(ND_ERR_ARG, "square accept needs 2 <= C <= 1024 (C=%d)", C);
    if (iter < -1) return nd_set_err(ND_ERR_ARG, "square accept needs iter >= -1 (iter=%d)", iter);
    hipLaunchKernelGGL(k_square_accept, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, scores, labels, margin_min, loss_min,
                       n_queries, flags, B, C, iter);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_square_commit(float* x_best, float* x_new, const int32_t* win, const int32_t* flags, int B, int Cin, int H, int W, int s,
                                void* stream) {
    if (!x_best || !x_new || !win || !flags) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (int rc = sq_check_image("square commit", B, Cin, H, W)) return rc;
    if (int rc = sq_check_side("square commit", H, W, s)) return rc;
    hipLaunchKernelGGL(k_square_commit, nd_image_grid(B, (size_t)Cin * s * s, SQ_MAX_BLOCKS), dim3(SQ_THREADS), 0, (hipStream_t)stream, x_best, x_new,
                       win, flags, Cin, H, W, s);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}
