// nd_skinny_kernel.hpp -- the weight-streaming kernel k_skinny and the launch plan that picks its instantiation.  Included by the three
// translation units that instantiate the family (csrc/nd_skinny_m{0,1,2}.hip, one MODE each) and by tools/ubench_skinny.hip; every other
// caller goes through nd_skinny.hpp.  gfx950 only.
#pragma once
#include <type_traits>
#include "nd_skinny.hpp"
#include "nd_math.hpp"
#include "nd_frag.hpp"
#include "nd_device.hpp"

#ifdef ND_WG_TIMING
__device__ long long* nd_dbg_times = nullptr;   // tools/ubench_skinny.hip: per-workgroup (start, loop end, end) clocks
#endif

#ifndef ND_PF_TWO
#define ND_PF_TWO 0
#endif
#ifndef ND_PF_LEAD
#define ND_PF_LEAD 0            // register stages between the cross-launch prefetch and the end of a wave's stream (~0.45 us each at M = 32)
#endif
// WORK DECOMPOSITION.  A workgroup never mixes members (it would have to stream two activation matrices and finishes
// 40 % late: measured).  Each member's nfr = ceil(N/16) 16-column output fragments go to wpm = gridDim.x / nm workgroups:
// base = nfr / wpm each, the first nfr % wpm of them one more.  NF (template) = the larger count; a workgroup holding
// NF - 1 fragments skips the last register slot (uniform branch).  The launcher picks wpm so that the grid is at most one
// workgroup per CU.  grid.y = 16*MT-row groups; grid.z = k-slabs (MODE 2 only).
// A wave keeps NF weight fragments and MT activation fragments per k-chunk in registers, so an activation fragment is
// loaded once per NF weight fragments.  The WAVES waves of a workgroup split K (interleaved groups of U chunks) and are
// summed through LDS in a fixed order => bitwise reproducible.
// MFMA 16x16x4 f32: A[i=l&15][k=l>>4] <- W rows, B[k=l>>4][j=l&15] <- x rows, D[i=4*(l>>4)+r][j=l&15];
// lane l's float4 holds k = 4*(l>>4)..+3 of a chunk and element jj feeds MFMA jj (same k permutation on
// both operands).
// H = 1: operands are frag32h (fp16), one v_mfma_f32_16x16x32_f16 per fragment pair and 32-column chunk.
#define ND_SKINNY_STATIC_LDS (60 * 1024)
__host__ __device__ constexpr int nd_skinny_red_bytes(int waves, int nf, int mt) { return waves * nf * mt * 1024; }
template <int MT, int NF, int WAVES, int U, int MODE, bool NT, int H = 0>
__global__ __launch_bounds__(WAVES * 64) void k_skinny(SkinnyInline di, const SkinnyDesc* __restrict__ table, int nm,
                                                       int M, int t, int cps) {
    const int tid = threadIdx.x, lane = tid & 63;
#ifdef ND_WG_TIMING
    const long long dbg_t0 = wall_clock64();
#endif
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: keeps stream addresses in SGPRs
    // both sources are read through the CONSTANT address space (scalar loads; a select between a kernarg and a generic pointer
    // would turn every descriptor access into a flat vector load): `di` is the first kernel argument = kernarg offset 0
    typedef const __attribute__((address_space(4))) char* nd_cbytes;
    const nd_cbytes dsrc = table ? (nd_cbytes)(uintptr_t)table : (nd_cbytes)__builtin_amdgcn_kernarg_segment_ptr();
    const int K = nd_ldc<SkinnyDesc>(dsrc).K, N = nd_ldc<SkinnyDesc>(dsrc).N;
    const int nch = H ? K >> 5 : K >> 4, nfr = (N + 15) >> 4, mtiles = (M + 15) >> 4;
    const int wpm = gridDim.x / nm;                               // workgroups per member
    const int g = blockIdx.x / wpm, j = blockIdx.x - g * wpm;     // member, workgroup inside the member
    const int base = nfr / wpm, rem = nfr - base * wpm;
    const int nact = base + (j < rem ? 1 : 0);                    // fragments this workgroup owns: NF or NF - 1
    const int fi0 = j * base + min(j, rem);                       // its first fragment inside the member
    const SkinnyDesc d = nd_ldc<SkinnyDesc>(dsrc + (size_t)g * sizeof(SkinnyDesc));
    const int c0 = MODE == 2 ? blockIdx.z * cps : 0;
    const int c1 = MODE == 2 ? min(c0 + cps, nch) : nch;
    const float* wp[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) wp[f] = d.w + ((size_t)min(fi0 + f, nfr - 1) * nch + c0) * 256;   // uniform; lane term added at the load
    const float* xp[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) xp[mt] = d.x + ((size_t)min((int)blockIdx.y * MT + mt, mtiles - 1) * nch + c0) * 256;
    f32x4 acc[NF][MT];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[f][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // Epilogue operands are requested NOW (registers; parked in LDS after the main loop): the scale/shift entries of the
    // workgroup's output columns and the lin4 rows of MODE 1.
    __shared__ float ssc[NF][16], ssh[NF][16];
    __shared__ float pws[MODE == 1 ? NF : 1][MODE == 1 ? 8 : 1][16];
    const int eact = d.act, eC = d.C, epacked = d.out_packed;
    float r_sc = 1.0f, r_sh = 0.0f, r_pw = 0.0f;
    if (MODE != 2) {
        // thread tid < NF*16 owns column (f = tid/16, nl = tid%16); thread tid < NF*C*16 owns lin4 entry (f, c, nl)
        if (tid < NF * 16) {
            const int n = min(min(fi0 + (tid >> 4), nfr - 1) * 16 + (tid & 15), N - 1);
            if (d.scale) r_sc = nd_ldg(d.scale + (size_t)t * N + n);
            if (d.shift) r_sh = nd_ldg(d.shift + (size_t)t * N + n);
        }
        // lin4 rows: one entry per thread when they fit (NF*C*16 <= threads), requested now and parked after the main loop;
        // otherwise (large C) fetched after the loop.  No load inside a loop of unknown trip count here: with one pending the
        // compiler can no longer count outstanding loads and degrades every wait of the main loop to vmcnt(0).
        // (an unconditional load on a clamped address, in the global address space: see nd_ldg)
        if (MODE == 1) {
            const int e = min(tid, NF * eC * 16 - 1);
            const int f = e / (eC * 16), c = (e / 16) % eC, nl = e & 15;
            const int n = min(min(fi0 + f, nfr - 1) * 16 + nl, N - 1);
            r_pw = nd_ldg(d.pw + (size_t)c * N + n);
        }
    }

    // cross-launch prefetch (d.pf): lane L of instruction q touches line (q*64 + L) % 8 of chunk (q*64 + L) / 8 of this wave's first
    // group in the next launch -- chunk ci = (fragment ci / U, chunk wave*U + ci % U of that fragment's row), 8 lines of 128 B each
    const float* pfp[2] = {nullptr, nullptr};
    if (MODE != 2 && NT && d.pf) {      // NT: the launch streams more than the Infinity Cache keeps (small launches run out of it: K = 1 measured 1.3 % slower with the prefetch)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int idx = q * 64 + lane, ci = min(idx >> 3, nact * U - 1), f = ci / U, u = ci - f * U;
            pfp[q] = d.pf + ((size_t)min(fi0 + f, nfr - 1) * nch + min(wave * U + u, nch - 1)) * 256 + (idx & 7) * 32;
        }
    }
    float pfv = 0.f;
    const int nck = max(c1 - c0, 0);
    const int ngroups = nck / U;     // full groups of U chunks
    const int ngw = ngroups > wave ? (ngroups - wave + WAVES - 1) / WAVES : 0;
    const int glast = ngroups > 0 ? ngroups - 1 : 0;

    // MAIN LOOP.  Two register stages (A, B), each a whole group of U chunks (NF weight + MT activation fragments), used
    // alternately with no copies: while the MFMAs of the current group run, the loads of the next one are issued, so every
    // wave keeps one group in flight under its arithmetic.  Scheduling barriers pin that order (left alone, the compiler
    // sinks the loads below the MFMAs to save registers and then waits on them at once).
    // FULL = false (a workgroup with NF - 1 fragments): the last fragment slot is neither loaded nor multiplied.
    const int lane4 = lane * 4;
    auto run = [&](auto ntc, auto fullc) {
        constexpr bool NTV = decltype(ntc)::value, FULL = decltype(fullc)::value;
        constexpr int NFA = FULL ? NF : (NF > 1 ? NF - 1 : 1);         // active fragment slots
        float4 wA[U][NFA], xA[U][MT], wB[U][NFA], xB[U][MT];
        auto LD = [&](float4 (&w)[U][NFA], float4 (&x)[U][MT], int grp) {
            const size_t go = (size_t)grp * U * 256;
#ifdef ND_SKINNY_ABLATE_W      // timing ablation only (variant library; results WRONG): every weight load of a wave goes to its FIRST register stage
            const size_t gow = (size_t)min(wave, glast) * U * 256;     // -- cache hits instead of fabric traffic, same instructions, same MFMAs
#else
            const size_t gow = go;
#endif
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int f = 0; f < NFA; ++f) w[u][f] = nd_ld16<NTV>(wp[f] + gow + u * 256 + lane4);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) x[u][mt] = nd_ld16<false>(xp[mt] + go + u * 256 + lane4);
            }
        };
        auto MMA = [&](const float4 (&w)[U][NFA], const float4 (&x)[U][MT]) {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int jj = 0; jj < (H ? 1 : 4); ++jj)
#pragma unroll
                    for (int f = 0; f < NFA; ++f)
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) {
                            if (H) {
                                acc[f][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(nd_as_h8(w[u][f]), nd_as_h8(x[u][mt]), acc[f][mt], 0, 0, 0);
                            } else {
                                const float wv = jj == 0 ? w[u][f].x : jj == 1 ? w[u][f].y : jj == 2 ? w[u][f].z : w[u][f].w;
                                const float xv = jj == 0 ? x[u][mt].x : jj == 1 ? x[u][mt].y : jj == 2 ? x[u][mt].z : x[u][mt].w;
                                acc[f][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv, xv, acc[f][mt], 0, 0, 0);
                            }
                        }
        };
        auto G = [&](int i) { return min(wave + i * WAVES, glast); };      // group of this wave's i-th turn (clamped)
        int i = 0;
        if (ngw > 0) LD(wA, xA, G(0));
        // Steady state.  The next stage's loads are spread through the current stage's MFMAs (one load per MR MFMAs), so the
        // matrix pipe never waits for the ~150 cycles of load issue: -3 us per launch against issuing them in a block first.
        constexpr int NL = U * (NFA + MT), NM = U * (H ? 1 : 4) * NFA * MT, MR = NM / NL > 0 ? NM / NL : 1;
#define ND_MIX()                                                                                     \
        _Pragma("unroll") for (int q_ = 0; q_ < NL; ++q_) {                                          \
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                                       \
            __builtin_amdgcn_sched_group_barrier(0x008, MR, 0);                                      \
        }                                                                                            \
        __builtin_amdgcn_sched_barrier(0);
        const int pf_at = ngw > ND_PF_LEAD ? (ngw - ND_PF_LEAD) & ~1 : 0;        // ~ND_PF_LEAD register stages before the end of the stream
        for (; i + 1 < ngw; i += 2) {
            if (MODE != 2 && pfp[0] && i == pf_at && ND_PF_LEAD > 0) {
                pfv += nd_ldg(pfp[0]) + nd_ldg(pfp[1]);
                if (ND_PF_TWO) pfv += nd_ldg(pfp[0] + (size_t)WAVES * U * 256) + nd_ldg(pfp[1] + (size_t)WAVES * U * 256);     // the wave's second group too
            }
            LD(wB, xB, G(i + 1));
            MMA(wA, xA);
            ND_MIX()
            LD(wA, xA, G(i + 2));          // i + 2 == ngw on the last pair of an even count: re-reads a valid group, unused
            MMA(wB, xB);
            ND_MIX()
        }
#undef ND_MIX
        if (ND_PF_LEAD == 0 && MODE != 2 && pfp[0]) pfv += nd_ldg(pfp[0]) + nd_ldg(pfp[1]);      // (variant: behind the last stage's loads)
        if (i < ngw) MMA(wA, xA);
    };
    const bool nt_here = NT && !d.keep;
    if (nact == NF) {
        if (nt_here) run(std::true_type{}, std::true_type{});
        else run(std::false_type{}, std::true_type{});
    } else {
        if (nt_here) run(std::true_type{}, std::false_type{});
        else run(std::false_type{}, std::false_type{});
    }
    // leftover chunks (chunk count not a multiple of U): chunk c goes to wave c % WAVES
    for (int c = ngroups * U + wave; c < nck; c += WAVES) {
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const float4 w4 = nd_ld16<false>(wp[f] + (size_t)c * 256 + lane4);
            const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const float4 x4 = nd_ld16<false>(xp[mt] + (size_t)c * 256 + lane4);
                const float xv[4] = {x4.x, x4.y, x4.z, x4.w};
                if (H) acc[f][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(nd_as_h8(w4), nd_as_h8(x4), acc[f][mt], 0, 0, 0);
                else {
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) acc[f][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[jj], xv[jj], acc[f][mt], 0, 0, 0);
                }
            }
        }
    }
#ifdef ND_WG_TIMING
    const long long dbg_t1 = wall_clock64();
#endif
    if (ND_PF_LEAD < 0 && MODE != 2 && pfp[0]) {                                  // (variant: at the start of the epilogue)
        pfv += nd_ldg(pfp[0]) + nd_ldg(pfp[1]);
        if (ND_PF_TWO) pfv += nd_ldg(pfp[0] + (size_t)WAVES * U * 256) + nd_ldg(pfp[1] + (size_t)WAVES * U * 256);
    }
    // park the epilogue operands (in registers since the prologue) in LDS; the first barrier below publishes them
    if (MODE != 2) {
        if (tid < NF * 16) { ssc[tid >> 4][tid & 15] = r_sc; ssh[tid >> 4][tid & 15] = r_sh; }
        if (MODE == 1) {
            if (NF * eC * 16 <= WAVES * 64) {
                if (tid < NF * eC * 16) {
                    const int f = tid / (eC * 16), nl = tid & 15;
                    pws[f][(tid / 16) % eC][nl] = (min(fi0 + f, nfr - 1) * 16 + nl < N) ? r_pw : 0.f;
                }
            } else {
                for (int e = tid; e < NF * eC * 16; e += WAVES * 64) {
                    const int f = e / (eC * 16), c = (e / 16) % eC, nl = e & 15;
                    const int n = min(fi0 + f, nfr - 1) * 16 + nl;
                    pws[f][c][nl] = n < N ? nd_ldg(d.pw + (size_t)c * N + n) : 0.f;
                }
            }
        }
    }

    // ---- all fragments at once: cross-wave reduction (fixed order) + epilogue, two barriers in total ----
    // red[w] holds wave w's accumulators in MFMA D order, element ((f*MT + mt)*4 + r)*64 + l  <->  n = 4*(l>>4)+r, m = l&15.
    // The reduced, activated value replaces plane 0 in place (same thread reads the four planes and writes plane 0).
    // (above 60 KiB -- five or six weight fragments against four or five row fragments -- the buffer is dynamic LDS: the launcher
    //  passes nd_skinny_dynlds<>() bytes; the smaller shapes keep their static array and their code)
    constexpr bool DYN = nd_skinny_red_bytes(WAVES, NF, MT) > ND_SKINNY_STATIC_LDS;
    __shared__ __attribute__((aligned(16))) float red_static[DYN ? 1 : WAVES][DYN ? 1 : NF * MT * 256];
    extern __shared__ __attribute__((aligned(16))) float red_dynamic[];
    float (*const red)[NF * MT * 256] = DYN ? reinterpret_cast<float (*)[NF * MT * 256]>(red_dynamic)
                                            : reinterpret_cast<float (*)[NF * MT * 256]>(&red_static[0][0]);
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wave][((f * MT + mt) * 4 + r) * 64 + lane] = acc[f][mt][r];
    __syncthreads();
#ifdef ND_WG_TIMING
    const long long dbg_t2 = wall_clock64();
    long long dbg_t3 = dbg_t2;
#endif
    float* const R = red[0];
    const int m0 = blockIdx.y * 16 * MT;
    if (MODE == 2) {
        // raw partial sums, [slab][Mp][Np]; lane l of a reduced tile owns n = 4*(l>>4)..+3 of row m = l&15
        const int Mp = mtiles * 16, Np = nfr * 16;
        for (int e = tid; e < nact * MT * 64; e += WAVES * 64) {
            const int f = e / (MT * 64), mt = (e >> 6) % MT, l = e & 63;
            const int mtg = blockIdx.y * MT + mt;
            if (mtg < mtiles) {
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int q = ((f * MT + mt) * 4 + r) * 64 + l;
                    float sum = red[0][q];
#pragma unroll
                    for (int w = 1; w < WAVES; ++w) sum += red[w][q];
                    v[r] = sum;
                }
                *reinterpret_cast<float4*>(d.part + ((size_t)blockIdx.z * Mp + mtg * 16 + (l & 15)) * Np + (fi0 + f) * 16 + 4 * (l >> 4)) =
                    make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    } else {
        // fully unrolled, no branches: with one wave per SIMD the only latency hiding is the instruction-level parallelism
        // of these NF*MT*256/threads independent activations (slots f >= nact hold zeros: computed, never stored further)
        static_assert((MT * 256) % (WAVES * 64) == 0, "epilogue assumes MT*256 is a multiple of the workgroup size");
        constexpr int EPF = MT * 256 / (WAVES * 64);        // elements per thread and fragment
        float ev[NF][EPF];
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int jq = 0; jq < EPF; ++jq) {
                const int q = f * MT * 256 + jq * WAVES * 64 + tid;
                float sum = red[0][q];
#pragma unroll
                for (int w = 1; w < WAVES; ++w) sum += red[w][q];
                const int nl = 4 * ((q & 63) >> 4) + ((q >> 6) & 3);
                ev[f][jq] = ssc[f][nl] * sum + ssh[f][nl];
            }
        // the activation is uniform: branch once, then a straight run of independent evaluations
        auto activate = [&](auto fn) {
#pragma unroll
            for (int f = 0; f < NF; ++f)
#pragma unroll
                for (int jq = 0; jq < EPF; ++jq) ev[f][jq] = fn(ev[f][jq]);
        };
        switch (eact) {
            case ND_ACT_SOFTPLUS: activate([](float v) { return nd_softplus(v); }); break;
            case ND_ACT_RELU: activate([](float v) { return v > 0.0f ? v : 0.0f; }); break;
            case ND_ACT_GELU: activate([](float v) { return 0.5f * v * (1.0f + nd_erf(v * 0.70710678118654752440f)); }); break;
            default: break;
        }
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int jq = 0; jq < EPF; ++jq) {
                const int q = f * MT * 256 + jq * WAVES * 64 + tid;
                const int nl = 4 * ((q & 63) >> 4) + ((q >> 6) & 3);
                R[q] = ((fi0 + f) * 16 + nl < N) ? ev[f][jq] : 0.f;
            }
        __syncthreads();
#ifdef ND_WG_TIMING
        dbg_t3 = wall_clock64();
#endif
        if (MODE == 0) {
            if (epacked == 2) {
                // frag32h: a fragment's 16 columns are k-groups (nfi&1)*2 + {0,1} of block (m-tile, nfi/2): lanes
                // 32*(nfi&1) .. +31 of it, 512 contiguous bytes per m-tile
                _Float16* outh = reinterpret_cast<_Float16*>(d.out);
                const int nch_o = N >> 5;
                for (int e = tid; e < nact * MT * 32; e += WAVES * 64) {
                    const int f = e / (MT * 32), mt = (e >> 5) % MT, L = e & 31, nfi = fi0 + f;
                    const int mtg = blockIdx.y * MT + mt;
                    if (mtg < mtiles) {
                        const float* tp = R + (f * MT + mt) * 256 + (L & 15) + 32 * (L >> 4);   // l0 = m + 16*(2*(L>>4)), l1 = l0 + 16
                        const f16x8 h = {(_Float16)tp[0], (_Float16)tp[64], (_Float16)tp[128], (_Float16)tp[192],
                                         (_Float16)tp[16], (_Float16)tp[80], (_Float16)tp[144], (_Float16)tp[208]};
                        *reinterpret_cast<f16x8*>(outh + ((size_t)mtg * nch_o + (nfi >> 1)) * 512 + ((nfi & 1) * 32 + L) * 8) = h;
                    }
                }
            } else if (epacked) {
                // the 16x16 block (m-tile, fragment) is one contiguous 1 KiB of the frag16 output
                for (int e = tid; e < nact * MT * 64; e += WAVES * 64) {
                    const int f = e / (MT * 64), mt = (e >> 6) % MT, L = e & 63;
                    const int mtg = blockIdx.y * MT + mt;
                    if (mtg < mtiles) {
                        const float* tp = R + (f * MT + mt) * 256 + L;
                        *reinterpret_cast<float4*>(d.out + ((size_t)mtg * nfr + fi0 + f) * 256 + L * 4) = make_float4(tp[0], tp[64], tp[128], tp[192]);
                    }
                }
            } else {
                for (int e = tid; e < nact * MT * 256; e += WAVES * 64) {
                    const int f = e / (MT * 256), ml = (e >> 4) % (16 * MT), nl = e & 15;
                    const int m = m0 + ml, n = (fi0 + f) * 16 + nl;
                    if (m < M && n < N) d.out[(size_t)m * N + n] = R[((f * MT + (ml >> 4)) * 4 + (nl & 3)) * 64 + (ml & 15) + 16 * (nl >> 2)];
                }
            }
        } else {
            for (int e = tid; e < nact * 16 * MT * eC; e += WAVES * 64) {
                const int f = e / (16 * MT * eC), ml = (e / eC) % (16 * MT), c = e % eC;
                const int m = m0 + ml;
                if (m < M) {
                    const float* tp = R + (f * MT + (ml >> 4)) * 256 + (ml & 15);
                    float sum = 0.f;
#pragma unroll
                    for (int nl = 0; nl < 16; ++nl) sum += pws[MODE == 1 ? f : 0][MODE == 1 ? c : 0][nl] * tp[(nl & 3) * 64 + 16 * (nl >> 2)];
                    d.part[((size_t)m * eC + c) * nfr + fi0 + f] = sum;
                }
            }
        }
    }
    // the prefetched values themselves are of no interest: a never-true use keeps the loads (and the compiler's own count of them) alive
    if (MODE != 2 && pfv == 1.2345678e30f && d.part) d.part[0] = pfv;
#ifdef ND_WG_TIMING
    if (tid == 0 && nd_dbg_times) {
        long long* q = nd_dbg_times + ((size_t)MODE * 8192 + blockIdx.x) * 3;      // one region per MODE: the last launch of each stays
        q[0] = dbg_t0; q[1] = dbg_t1; q[2] = wall_clock64();
        long long* q2 = nd_dbg_times + ((size_t)MODE * 8192 + 4096 + blockIdx.x) * 3;
        q2[0] = dbg_t2; q2[1] = dbg_t3; q2[2] = 0;
    }
#endif
}

// Geometry.  Measured (tools/ubench_skinny.hip, "sx" study, 5 x 67 MB at M = 32): weight stream alone 51 us, f32 MFMAs alone
// 40 us; together 80 us with 16 waves per CU, 66 us with 8, 57 us (min 51) with FOUR -- one wave per SIMD, each keeping two
// register stages so its own loads fly under its own MFMAs.  More waves per SIMD make the two overlap worse, not better.
// So: 4-wave workgroups, at most one per CU, every member's fragments spread evenly over its share of them (5 or 6 each at
// K = 5 members: 255 workgroups), U chunks per stage chosen to keep ~8-16 KiB per wave in flight.  Weights larger than what the 256 MiB Infinity Cache keeps
// across consecutive steps are streamed with nontemporal loads.
// MODE 2 (split-K): S k-slabs in grid.z so that (fragment groups) x (row groups) x S ~ 256 workgroups.
template <int MODE>
static inline SkinnyLaunch nd_skinny_launch_impl(int K, int N, int M, int nm, int half) {
    const int mt = nd_pick_mt(M);
    const int nfr = (N + 15) / 16, nch = half ? K / 32 : K / 16;
    const int mgroups = (M + 16 * mt - 1) / (16 * mt);
    const int nfmax = 6;                           // register budget (accumulators + two stages); LDS: see nd_skinny_red_bytes
    const int ncu = nd_num_cus();
    // workgroups per member: as many as keep the grid within one workgroup per CU, but no workgroup above nfmax fragments
    int wpm = ncu / nm;
    if (wpm < 1) wpm = 1;
    if (wpm > nfr) wpm = nfr;
    while ((nfr + wpm - 1) / wpm > nfmax) ++wpm;
    int S = 1, cps = nch;
    if (MODE == 2) {
        // split-K: k-slabs fill the CUs, so fragments per workgroup can stay high (each workgroup streams the x of its
        // slab once per NF weight fragments: at NF = 1 that is twice the weight bytes).  Pick (workgroups per member, S)
        // by cost = (1 + 0.3*MT/nf) / (fraction of the 256 CUs busy).
        double best = 1e30;
        int bw = wpm, bs = 1;
        for (int nfc = nfmax; nfc >= 1; --nfc) {
            const int w = (nfr + nfc - 1) / nfc;
            const int wgs = nm * w * mgroups;
            int sc = wgs >= ncu ? 1 : ncu / wgs;
            while (sc > 1 && nch / sc < 64) --sc;          // keep every slab >= 64 chunks deep
            const long tot = (long)wgs * sc;
            const double util = tot >= ncu ? (double)tot / ((double)ncu * ((tot + ncu - 1) / ncu)) : tot / (double)ncu;
            const double nfe = (double)nfr / w;
            const double cost = (1.0 + 0.3 * mt / nfe) / util;
            if (cost < best - 1e-9) { best = cost; bw = w; bs = sc; }
        }
        wpm = bw; S = bs;
        cps = (nch + S - 1) / S;
        S = (nch + cps - 1) / cps;
    }
    const int nf = (nfr + wpm - 1) / wpm;          // = base + (nfr % wpm != 0): the kernel's fragment slots
    const int gx = nm * wpm;
    const bool nt = (double)nm * N * (double)K * (half ? 2.0 : 4.0) > 160e6;
    SkinnyLaunch L{nullptr, dim3(gx, mgroups, S), dim3(256), cps, S, 0u, hipSuccess};
    // One table of the family: [row fragments MT = 1, 2, 4, 5][weight fragments NF - 1][operand type][load policy].  U, the chunks per
    // register stage, is 4 for the narrow shapes (MT <= 2 and NF <= 2) and 2 elsewhere; four waves everywhere.
#define ND_SK(MTV, NFV, UV)                                                                                  \
    {{(void*)k_skinny<MTV, NFV, 4, UV, MODE, false, 0>, (void*)k_skinny<MTV, NFV, 4, UV, MODE, true, 0>},    \
     {(void*)k_skinny<MTV, NFV, 4, UV, MODE, false, 1>, (void*)k_skinny<MTV, NFV, 4, UV, MODE, true, 1>}}
#define ND_SK_ROW(MTV, UN) {ND_SK(MTV, 1, UN), ND_SK(MTV, 2, UN), ND_SK(MTV, 3, 2), ND_SK(MTV, 4, 2), ND_SK(MTV, 5, 2), ND_SK(MTV, 6, 2)}
    static void* const fns[4][6][2][2] = {ND_SK_ROW(1, 4), ND_SK_ROW(2, 4), ND_SK_ROW(4, 2), ND_SK_ROW(5, 2)};
#undef ND_SK_ROW
#undef ND_SK
    L.fn = fns[mt == 1 ? 0 : mt == 2 ? 1 : mt == 4 ? 2 : 3][(nf >= 1 && nf <= 5 ? nf : 6) - 1][half ? 1 : 0][nt ? 1 : 0];
    if (nd_skinny_red_bytes(4, nf, mt) > ND_SKINNY_STATIC_LDS) {
        L.lds = (unsigned)nd_skinny_red_bytes(4, nf, mt);
        L.err = nd_allow_dynamic_lds(L.fn, L.lds);
    }
    return L;
}
