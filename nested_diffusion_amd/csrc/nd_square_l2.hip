// nd_square_l2.hip -- the attack side of a Square-attack query in the L2 threat model (Andriushchenko et al.; the L2 branch of autoattack's
// square.py); the listing is in nested_diffusion_amd/square.py.  gfx950 only, wave64, all arithmetic fp32.
//   k_sl2_init_sum     per-workgroup partial of sum D0^2, D0 the tiled eta(s0) start (recomputed from Philox, never stored)
//   k_sl2_init_write   finishes ||D0||, x_best = x_new = clip(x0 + D0 / (1e-12 + ||D0||) * eps, lo, hi)
//   k_sl2_sums         per active row, over the whole image: the windows of this query drawn from Philox (win), and the partials of the
//                      four masked sums of D^2, D = x_best - x0: over w1, over everything, over w1 u w2, outside w1 u w2
//   k_sl2_u            finishes those four; over w1: u = sigma_c * eta_t + D / (1e-12 + n_w1), the partial of sum u^2
//   k_sl2_new          finishes S_u; over w1: D' = u / (1e-12 + n_u) * scale (u recomputed), the partial of sum D'^2
//   k_sl2_write        finishes S_new; over the whole image: x_new = clip(x0 + D' / (1e-12 + n') * eps, lo, hi), D' recomputed per element
//   k_sl2_commit       accepted rows: x_best = x_new over the whole image
//
// A propose is four launches on one stream: each pass needs a per-image scalar that the pass before it reduces, and stream order between
// launches is the barrier.  Row sums have the fixed shape of nd_attack.hpp (one partial per workgroup, a finishing pass with the same xor
// tree, no floating-point atomics).  A wave owns one image row (c, h) -- or one window row (c, dh) -- at a time; a lane owns whole quads of
// four consecutive w and adds their terms in ascending w.  Where W % 4 == 0 and every image is 16-byte aligned a quad is one dwordx4
// access, otherwise four scalar ones: the terms and their order are the same, so a sum has the same bits either way, at every batch size
// and at every position in the batch.  Whether an element lies in w1 or w2 is decided per row for h and by two unsigned compares for w:
// no division per element.
#include "nd_attack.hpp"
#include "nd_philox.hpp"

// every operation below is one rounded fp32 op in the listed order: a float32 restatement on the host reproduces every array bit for bit
#pragma clang fp contract(off)

namespace {

constexpr int SL_THREADS = ND_ATTACK_THREADS;
constexpr int SL_WAVES = SL_THREADS / 64;
constexpr int SL_MIN_DIM = 5, SL_MAX_DIM = 4096;     // Cin * H * W <= 2^29: every in-image offset stays inside int
constexpr int SL_PARTS = ND_L2_MAX_PARTS;
// the partials of image b and sum k (ND_SQUARE_L2_S_*): ws + (b * ND_SQUARE_L2_SUMS + k) * SL_PARTS
__device__ __forceinline__ float* sl_part(float* ws, int b, int k) { return ws + ((size_t)b * ND_SQUARE_L2_SUMS + k) * SL_PARTS; }

struct SlQuery {
    int vh1, vw1, vh2, vw2;
    uint32_t signs;
    bool transpose;
};

__device__ __forceinline__ SlQuery sl_draw(uint32_t image, uint32_t iter, uint32_t restart, uint64_t seed, int H, int W, int s) {
    uint32_t p[4] = {image, iter, restart, ND_SQUARE_L2_STEP_TAG};
    nd_philox4x32_10(p, (uint32_t)seed, (uint32_t)(seed >> 32));
    uint32_t q[4] = {image, iter, restart, ND_SQUARE_L2_SIGN_TAG};
    nd_philox4x32_10(q, (uint32_t)seed, (uint32_t)(seed >> 32));
    SlQuery r;
    r.vh1 = (int)__umulhi(p[0], (uint32_t)(H - s + 1));          // (uint64(word) * (H - s + 1)) >> 32: in [0, H - s]
    r.vw1 = (int)__umulhi(p[1], (uint32_t)(W - s + 1));
    r.vh2 = (int)__umulhi(p[2], (uint32_t)(H - s + 1));
    r.vw2 = (int)__umulhi(p[3], (uint32_t)(W - s + 1));
    r.signs = q[0];
    r.transpose = (q[1] >> 31) != 0;
    return r;
}

__device__ __forceinline__ bool sl_in(int v, int lo, int s) { return (unsigned)(v - lo) < (unsigned)s; }

// the quad at w of a row of W elements; elements past the row's end read as 0
template <bool VEC>
__device__ __forceinline__ float4 sl_load4(const float* __restrict__ row, int w, int W) {
    if (VEC) return *reinterpret_cast<const float4*>(row + w);
    float4 v;
    v.x = row[w];
    v.y = w + 1 < W ? row[w + 1] : 0.f;
    v.z = w + 2 < W ? row[w + 2] : 0.f;
    v.w = w + 3 < W ? row[w + 3] : 0.f;
    return v;
}

template <bool VEC>
__device__ __forceinline__ void sl_store4(float* __restrict__ row, int w, int W, float4 v) {
    if (VEC) {
        *reinterpret_cast<float4*>(row + w) = v;
        return;
    }
    row[w] = v.x;
    if (w + 1 < W) row[w + 1] = v.y;
    if (w + 2 < W) row[w + 2] = v.z;
    if (w + 3 < W) row[w + 3] = v.w;
}

// ---- the start ------------------------------------------------------------------------------------------------------------------------
struct SlTiles {
    int s0, nh, nw, oh, ow;
};

__device__ __forceinline__ SlTiles sl_tiles(int H, int W, int s0) {
    SlTiles t;
    t.s0 = s0; t.nh = H / s0; t.nw = W / s0;
    t.oh = (H - t.nh * s0) / 2; t.ow = (W - t.nw * s0) / 2;
    return t;
}

// D0 at (c, h, w) of the image whose low index word is `image`: sigma(c, tile) * eta_t(s0) inside the tiled region, 0 outside it
__device__ __forceinline__ float sl_d0(const float* __restrict__ eta0, const SlTiles& t, uint32_t image, int c, int h, int w, uint64_t seed,
                                       uint32_t restart) {
    const int hh = h - t.oh, ww = w - t.ow;
    if (hh < 0 || ww < 0 || hh >= t.nh * t.s0 || ww >= t.nw * t.s0) return 0.f;
    const int th = hh / t.s0, tw = ww / t.s0, i = hh - th * t.s0, j = ww - tw * t.s0;
    uint32_t q[4] = {image, (uint32_t)(th * t.nw + tw), restart, ND_SQUARE_L2_INIT_TAG};
    nd_philox4x32_10(q, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float sigma = ((q[0] >> c) & 1u) ? 1.0f : -1.0f;
    const float e = (q[1] >> 31) ? eta0[j * t.s0 + i] : eta0[i * t.s0 + j];
    return sigma * e;
}

// grid (parts, B): a wave per image row, a lane per w (scalar: the start runs once per restart)
__global__ __launch_bounds__(SL_THREADS) void k_sl2_init_sum(const int64_t* __restrict__ index, const float* __restrict__ eta0, float* __restrict__ ws,
                                                             int Cin, int H, int W, int s0, uint64_t seed, uint32_t restart) {
    __shared__ float sh[4];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t image = (uint32_t)index[b];
    const SlTiles t = sl_tiles(H, W, s0);
    float acc = 0.f;
    for (int r = blockIdx.x * SL_WAVES + wave; r < Cin * H; r += gridDim.x * SL_WAVES) {
        const int c = r / H, h = r - c * H;
        for (int w = lane; w < W; w += 64) {
            const float d = sl_d0(eta0, t, image, c, h, w, seed, restart);
            acc += d * d;
        }
    }
    acc = l2_block_sum(acc, sh);
    if (threadIdx.x == 0) sl_part(ws, b, 0)[blockIdx.x] = acc;
}

__global__ __launch_bounds__(SL_THREADS) void k_sl2_init_write(const float* __restrict__ x0, const int64_t* __restrict__ index,
                                                               const float* __restrict__ eta0, float* __restrict__ x_best, float* __restrict__ x_new,
                                                               float* __restrict__ sums, float* __restrict__ ws, int Cin, int H, int W, int s0,
                                                               uint64_t seed, uint32_t restart, float eps, float lo, float hi) {
    __shared__ float sh[4];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t image = (uint32_t)index[b];
    const SlTiles t = sl_tiles(H, W, s0);
    const float S = l2_finish(sl_part(ws, b, 0), gridDim.x, sh);
    if (blockIdx.x == 0 && threadIdx.x == 0) sums[b] = S;
    const float den = 1e-12f + sqrtf(S);
    const size_t img = (size_t)b * Cin * H * W;
    for (int r = blockIdx.x * SL_WAVES + wave; r < Cin * H; r += gridDim.x * SL_WAVES) {
        const int c = r / H, h = r - c * H;
        const size_t row = img + (size_t)r * W;
        for (int w = lane; w < W; w += 64) {
            const float d = sl_d0(eta0, t, image, c, h, w, seed, restart);
            const float v = nd_clampf(x0[row + w] + (d / den) * eps, lo, hi);
            x_best[row + w] = v;
            x_new[row + w] = v;
        }
    }
}

// ---- a query --------------------------------------------------------------------------------------------------------------------------
// A frozen row (margin_min > 0 is false: <= 0, -0.0 and NaN alike) returns before any write in every kernel; the test is uniform over the
// workgroup, so the barriers of the sums below are never split.

// grid (parts of the image, B)
template <bool VEC>
__global__ __launch_bounds__(SL_THREADS) void k_sl2_sums(const float* __restrict__ x0, const float* __restrict__ x_best, const int64_t* __restrict__ index,
                                                         const float* __restrict__ margin_min, int32_t* __restrict__ win, float* __restrict__ ws,
                                                         int Cin, int H, int W, int s, uint32_t iter, uint64_t seed, uint32_t restart) {
    __shared__ float sh[4];
    const int b = blockIdx.y;
    if (!(margin_min[b] > 0.0f)) return;
    const SlQuery q = sl_draw((uint32_t)index[b], iter, restart, seed, H, W, s);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        win[4 * b] = q.vh1; win[4 * b + 1] = q.vw1; win[4 * b + 2] = q.vh2; win[4 * b + 3] = q.vw2;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, quads = (W + 3) >> 2;
    const size_t img = (size_t)b * Cin * H * W;
    float a_w1 = 0.f, a_all = 0.f, a_mask = 0.f, a_out = 0.f;
    for (int r = blockIdx.x * SL_WAVES + wave; r < Cin * H; r += gridDim.x * SL_WAVES) {
        const int h = r % H;
        const bool h1 = sl_in(h, q.vh1, s), h2 = sl_in(h, q.vh2, s);
        const float *xr = x0 + img + (size_t)r * W, *br = x_best + img + (size_t)r * W;
        for (int k = lane; k < quads; k += 64) {
            const int w = k << 2;
            const float4 x = sl_load4<VEC>(xr, w, W), xb = sl_load4<VEC>(br, w, W);
            const float d[4] = {xb.x - x.x, xb.y - x.y, xb.z - x.z, xb.w - x.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float sq = d[e] * d[e];                    // past the row's end: 0, and a sum of squares plus 0 keeps its bits
                const bool m1 = h1 && sl_in(w + e, q.vw1, s), m = m1 || (h2 && sl_in(w + e, q.vw2, s));
                a_all += sq;
                a_w1 += m1 ? sq : 0.f;
                a_mask += m ? sq : 0.f;
                a_out += m ? 0.f : sq;
            }
        }
    }
    a_w1 = l2_block_sum(a_w1, sh);
    a_all = l2_block_sum(a_all, sh);
    a_mask = l2_block_sum(a_mask, sh);
    a_out = l2_block_sum(a_out, sh);
    if (threadIdx.x == 0) {
        sl_part(ws, b, ND_SQUARE_L2_S_W1)[blockIdx.x] = a_w1;
        sl_part(ws, b, ND_SQUARE_L2_S_ALL)[blockIdx.x] = a_all;
        sl_part(ws, b, ND_SQUARE_L2_S_MASK)[blockIdx.x] = a_mask;
        sl_part(ws, b, ND_SQUARE_L2_S_OUT)[blockIdx.x] = a_out;
    }
}

// what the window passes and the write need of a row, workgroup-uniform
struct SlRow {
    float den_w1, den_u, scale;
};

// u at window element (dh, dw) of channel c, D its x_best - x0
__device__ __forceinline__ float sl_u(const float* __restrict__ eta, const SlQuery& q, int s, int c, int dh, int dw, float D, float den_w1) {
    const float sigma = ((q.signs >> c) & 1u) ? 1.0f : -1.0f;
    const float e = q.transpose ? eta[dw * s + dh] : eta[dh * s + dw];
    return sigma * e + D / den_w1;
}

// scale = sqrt(max(eps * eps - n_img * n_img, 0) / Cin + n_mask * n_mask)
__device__ __forceinline__ float sl_scale(float S_all, float S_mask, float eps, int Cin) {
    const float n_img = sqrtf(S_all), n_mask = sqrtf(S_mask);
    return sqrtf(fmaxf(eps * eps - n_img * n_img, 0.f) / (float)Cin + n_mask * n_mask);
}

// grid (parts of the window, B): a wave per window row (c, dh), a lane per dw; windows start anywhere, so every access is scalar.
// FINAL = false: the partial of sum u^2.  FINAL = true: the partial of sum D'^2 over w1, D' = u / (1e-12 + n_u) * scale.
template <bool FINAL>
__global__ __launch_bounds__(SL_THREADS) void k_sl2_window(const float* __restrict__ x0, const float* __restrict__ x_best, const int64_t* __restrict__ index,
                                                           const float* __restrict__ margin_min, const float* __restrict__ eta, float* sums,
                                                           float* __restrict__ ws, int image_parts, int B, int Cin, int H, int W, int s, uint32_t iter,
                                                           uint64_t seed, uint32_t restart, float eps) {
    __shared__ float sh[4];
    const int b = blockIdx.y;
    if (!(margin_min[b] > 0.0f)) return;
    const SlQuery q = sl_draw((uint32_t)index[b], iter, restart, seed, H, W, s);
    SlRow row;
    if (!FINAL) {
        float S[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) S[k] = l2_finish(sl_part(ws, b, k), image_parts, sh);
        if (blockIdx.x == 0 && threadIdx.x == 0)
            for (int k = 0; k < 4; ++k) sums[(size_t)k * B + b] = S[k];
        row.den_w1 = 1e-12f + sqrtf(S[ND_SQUARE_L2_S_W1]);
        row.den_u = row.scale = 0.f;
    } else {
        const float S_u = l2_finish(sl_part(ws, b, ND_SQUARE_L2_S_U), gridDim.x, sh);
        if (blockIdx.x == 0 && threadIdx.x == 0) sums[(size_t)ND_SQUARE_L2_S_U * B + b] = S_u;
        row.den_w1 = 1e-12f + sqrtf(sums[(size_t)ND_SQUARE_L2_S_W1 * B + b]);
        row.den_u = 1e-12f + sqrtf(S_u);
        row.scale = sl_scale(sums[(size_t)ND_SQUARE_L2_S_ALL * B + b], sums[(size_t)ND_SQUARE_L2_S_MASK * B + b], eps, Cin);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t img = (size_t)b * Cin * H * W;
    float acc = 0.f;
    for (int r = blockIdx.x * SL_WAVES + wave; r < Cin * s; r += gridDim.x * SL_WAVES) {
        const int c = r / s, dh = r - c * s;
        const size_t o = img + ((size_t)c * H + (q.vh1 + dh)) * W + q.vw1;
        for (int dw = lane; dw < s; dw += 64) {
            const float u = sl_u(eta, q, s, c, dh, dw, x_best[o + dw] - x0[o + dw], row.den_w1);
            const float v = FINAL ? (u / row.den_u) * row.scale : u;
            acc += v * v;
        }
    }
    acc = l2_block_sum(acc, sh);
    if (threadIdx.x == 0) sl_part(ws, b, FINAL ? ND_SQUARE_L2_S_NEW : ND_SQUARE_L2_S_U)[blockIdx.x] = acc;
}

// grid (parts of the image, B): the whole of x_new[b]
template <bool VEC>
__global__ __launch_bounds__(SL_THREADS) void k_sl2_write(const float* __restrict__ x0, const float* __restrict__ x_best, float* __restrict__ x_new,
                                                          const int64_t* __restrict__ index, const float* __restrict__ margin_min,
                                                          const float* __restrict__ eta, float* sums, float* __restrict__ ws, int window_parts, int B,
                                                          int Cin, int H, int W, int s, uint32_t iter, uint64_t seed, uint32_t restart, float eps,
                                                          float lo, float hi) {
    __shared__ float sh[4];
    const int b = blockIdx.y;
    if (!(margin_min[b] > 0.0f)) return;
    const SlQuery q = sl_draw((uint32_t)index[b], iter, restart, seed, H, W, s);
    const float S_new = l2_finish(sl_part(ws, b, ND_SQUARE_L2_S_NEW), window_parts, sh);
    if (blockIdx.x == 0 && threadIdx.x == 0) sums[(size_t)ND_SQUARE_L2_S_NEW * B + b] = S_new;
    SlRow row;
    row.den_w1 = 1e-12f + sqrtf(sums[(size_t)ND_SQUARE_L2_S_W1 * B + b]);
    row.den_u = 1e-12f + sqrtf(sums[(size_t)ND_SQUARE_L2_S_U * B + b]);
    row.scale = sl_scale(sums[(size_t)ND_SQUARE_L2_S_ALL * B + b], sums[(size_t)ND_SQUARE_L2_S_MASK * B + b], eps, Cin);
    const float den = 1e-12f + sqrtf(sums[(size_t)ND_SQUARE_L2_S_OUT * B + b] + S_new);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, quads = (W + 3) >> 2;
    const size_t img = (size_t)b * Cin * H * W;
    for (int r = blockIdx.x * SL_WAVES + wave; r < Cin * H; r += gridDim.x * SL_WAVES) {
        const int c = r / H, h = r - c * H;
        const bool h1 = sl_in(h, q.vh1, s), h2 = sl_in(h, q.vh2, s);
        const float *xr = x0 + img + (size_t)r * W, *br = x_best + img + (size_t)r * W;
        float* nr = x_new + img + (size_t)r * W;
        for (int k = lane; k < quads; k += 64) {
            const int w = k << 2;
            const float4 x = sl_load4<VEC>(xr, w, W), xb = sl_load4<VEC>(br, w, W);
            const float xs[4] = {x.x, x.y, x.z, x.w}, bs[4] = {xb.x, xb.y, xb.z, xb.w};
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float D = bs[e] - xs[e];
                float dn = D;
                if (h1 && sl_in(w + e, q.vw1, s))                    // w1 wins where the windows overlap
                    dn = (sl_u(eta, q, s, c, h - q.vh1, w + e - q.vw1, D, row.den_w1) / row.den_u) * row.scale;
                else if (h2 && sl_in(w + e, q.vw2, s))
                    dn = 0.f;
                o[e] = nd_clampf(xs[e] + (dn / den) * eps, lo, hi);
            }
            sl_store4<VEC>(nr, w, W, float4{o[0], o[1], o[2], o[3]});
        }
    }
}

// grid (blocks per image, B): ACTIVE | ACCEPT rows copy the whole image, the others do nothing
template <bool VEC>
__global__ __launch_bounds__(SL_THREADS) void k_sl2_commit(float* __restrict__ x_best, const float* __restrict__ x_new, const int32_t* __restrict__ flags,
                                                           size_t per_image) {
    const int b = blockIdx.y;
    if ((flags[b] & (ND_SQUARE_ACTIVE | ND_SQUARE_ACCEPT)) != (ND_SQUARE_ACTIVE | ND_SQUARE_ACCEPT)) return;
    const size_t img = (size_t)b * per_image, step = (size_t)gridDim.x * SL_THREADS;
    if (VEC) {
        const float4* src = reinterpret_cast<const float4*>(x_new + img);
        float4* dst = reinterpret_cast<float4*>(x_best + img);
        for (size_t i = (size_t)blockIdx.x * SL_THREADS + threadIdx.x; i < per_image / 4; i += step) dst[i] = src[i];
    } else {
        for (size_t i = (size_t)blockIdx.x * SL_THREADS + threadIdx.x; i < per_image; i += step) x_best[img + i] = x_new[img + i];
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
int sl_check_image(const char* what, int B, int Cin, int H, int W) {
    if (B < 1 || B > 65535) return nd_set_err(ND_ERR_ARG, "%s needs 1 <= B <= 65535 (B=%d)", what, B);
    if (Cin < 1 || Cin > 32) return nd_set_err(ND_ERR_ARG, "%s needs 1 <= Cin <= 32 (Cin=%d)", what, Cin);
    if (H < SL_MIN_DIM || W < SL_MIN_DIM || H > SL_MAX_DIM || W > SL_MAX_DIM)
        return nd_set_err(ND_ERR_ARG, "%s needs %d <= H, W <= %d (H=%d, W=%d)", what, SL_MIN_DIM, SL_MAX_DIM, H, W);
    return ND_OK;
}

// a wave per row: ceil(rows / 4) workgroups, at most SL_PARTS; a function of the row count alone
unsigned sl_parts(int rows) { return nd_blocks_per_image((size_t)rows * 64, SL_PARTS); }

bool sl_vec(int W, const void* const* p, int n) {
    if (W % 4) return false;
    for (int i = 0; i < n; ++i)
        if (nd_misaligned(p[i], 15)) return false;
    return true;
}

}  // namespace

extern "C" size_t nd_square_l2_ws_floats(int Cin, int H, int W) {
    if (Cin < 1 || Cin > 32 || H < SL_MIN_DIM || W < SL_MIN_DIM || H > SL_MAX_DIM || W > SL_MAX_DIM) return 0;
    return (size_t)ND_SQUARE_L2_SUMS * SL_PARTS;
}

extern "C" int nd_square_l2_init(const float* x0, const int64_t* index, const float* eta0, float* x_best, float* x_new, float* sums, float* ws,
                                 int B, int Cin, int H, int W, int s0, uint64_t seed, uint32_t restart, float eps, float lo, float hi,
                                 void* stream) {
    if (!x0 || !index || !eta0 || !x_best || !x_new || !sums || !ws) return nd_set_err(ND_ERR_ARG, "nd_square_l2_init: NULL tensor");
    if (int rc = sl_check_image("square L2 init", B, Cin, H, W)) return rc;
    if (s0 != (H < W ? H : W) / 5) return nd_set_err(ND_ERR_ARG, "square L2 init needs s0 = min(H, W) / 5 (s0=%d, H=%d, W=%d)", s0, H, W);
    const dim3 grid(sl_parts(Cin * H), (unsigned)B), block(SL_THREADS);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_sl2_init_sum, grid, block, 0, st, index, eta0, ws, Cin, H, W, s0, seed, restart);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_sl2_init_write, grid, block, 0, st, x0, index, eta0, x_best, x_new, sums, ws, Cin, H, W, s0, seed, restart, eps, lo, hi);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_square_l2_propose(const float* x0, const float* x_best, float* x_new, const int64_t* index, const float* margin_min,
                                    const float* eta, int32_t* win, float* sums, float* ws, int B, int Cin, int H, int W, int s, int iter,
                                    uint64_t seed, uint32_t restart, float eps, float lo, float hi, void* stream) {
    if (!x0 || !x_best || !x_new || !index || !margin_min || !eta || !win || !sums || !ws)
        return nd_set_err(ND_ERR_ARG, "nd_square_l2_propose: NULL tensor");
    if (int rc = sl_check_image("square L2 propose", B, Cin, H, W)) return rc;
    if (s < 3 || !(s & 1) || s > H || s > W)
        return nd_set_err(ND_ERR_ARG, "square L2 propose needs an odd s, 3 <= s <= min(H, W) (s=%d, H=%d, W=%d)", s, H, W);
    if (iter < 0) return nd_set_err(ND_ERR_ARG, "square L2 propose needs iter >= 0 (iter=%d)", iter);
    if (x_new == x0 || x_new == x_best) return nd_set_err(ND_ERR_ARG, "square L2 propose writes x_new while it reads x0 and x_best: three arrays");
    const void* ptrs[] = {x0, x_best, x_new};
    const bool vec = sl_vec(W, ptrs, 3);
    const unsigned image_parts = sl_parts(Cin * H), window_parts = sl_parts(Cin * s);
    const dim3 ig(image_parts, (unsigned)B), wg(window_parts, (unsigned)B), block(SL_THREADS);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t it = (uint32_t)iter;
    if (vec)
        hipLaunchKernelGGL((k_sl2_sums<true>), ig, block, 0, st, x0, x_best, index, margin_min, win, ws, Cin, H, W, s, it, seed, restart);
    else
        hipLaunchKernelGGL((k_sl2_sums<false>), ig, block, 0, st, x0, x_best, index, margin_min, win, ws, Cin, H, W, s, it, seed, restart);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((k_sl2_window<false>), wg, block, 0, st, x0, x_best, index, margin_min, eta, sums, ws, (int)image_parts, B, Cin, H, W, s, it,
                       seed, restart, eps);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((k_sl2_window<true>), wg, block, 0, st, x0, x_best, index, margin_min, eta, sums, ws, (int)image_parts, B, Cin, H, W, s, it,
                       seed, restart, eps);
    HIP_CHECK(hipGetLastError());
    if (vec)
        hipLaunchKernelGGL((k_sl2_write<true>), ig, block, 0, st, x0, x_best, x_new, index, margin_min, eta, sums, ws, (int)window_parts, B, Cin, H,
                           W, s, it, seed, restart, eps, lo, hi);
    else
        hipLaunchKernelGGL((k_sl2_write<false>), ig, block, 0, st, x0, x_best, x_new, index, margin_min, eta, sums, ws, (int)window_parts, B, Cin, H,
                           W, s, it, seed, restart, eps, lo, hi);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_square_l2_commit(float* x_best, const float* x_new, const int32_t* flags, int B, size_t per_image, void* stream) {
    if (!x_best || !x_new || !flags) return nd_set_err(ND_ERR_ARG, "nd_square_l2_commit: NULL tensor");
    if (B < 1 || B > 65535) return nd_set_err(ND_ERR_ARG, "square L2 commit needs 1 <= B <= 65535 (B=%d)", B);
    if (per_image < (size_t)SL_MIN_DIM * SL_MIN_DIM || per_image > (size_t)32 * SL_MAX_DIM * SL_MAX_DIM)
        return nd_set_err(ND_ERR_ARG, "square L2 commit needs 25 <= per_image <= 32 * 4096 * 4096 (per_image=%zu)", per_image);
    if (x_best == x_new) return nd_set_err(ND_ERR_ARG, "square L2 commit copies x_new into x_best: two arrays");
    const bool vec = per_image % 4 == 0 && !nd_misaligned(x_best, 15) && !nd_misaligned(x_new, 15);
    const dim3 grid = nd_image_grid(B, vec ? per_image / 4 : per_image, 1024), block(SL_THREADS);
    if (vec)
        hipLaunchKernelGGL((k_sl2_commit<true>), grid, block, 0, (hipStream_t)stream, x_best, x_new, flags, per_image);
    else
        hipLaunchKernelGGL((k_sl2_commit<false>), grid, block, 0, (hipStream_t)stream, x_best, x_new, flags, per_image);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}
