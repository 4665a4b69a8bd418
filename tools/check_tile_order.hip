// check_tile_order.hip -- the tile order of the LDS-tiled kernels (csrc/nd_tile.hpp: nd_xcd_run, nd_tile_decode, nd_slab_begin / nd_slab_end)
// walked on the host as a stand-alone program: plain integer arithmetic, no HIP call, no GPU.  Build (host pass only) and run:
//   hipcc --cuda-host-only -O1 -g -std=c++17 tools/check_tile_order.hip -o tools/bin/check_tile_order && tools/bin/check_tile_order
// or under the host sanitizers (CPU only, never on a GPU box):
//   hipcc --cuda-host-only -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined tools/check_tile_order.hip -o tools/bin/check_tile_order
//   ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=halt_on_error=1 tools/bin/check_tile_order
#include <stdio.h>
#include <vector>
#include "../nested_diffusion_amd/csrc/nd_tile.hpp"

static int g_failed = 0;
#define EXPECT(cond, ...)                                                                                 \
    do {                                                                                                  \
        if (!(cond)) { if (g_failed < 20) { printf("FAIL  %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } ++g_failed; } \
    } while (0)

// nd_xcd_run is a bijection of [0, total), and the blocks of one XCD (bid % 8, in dispatch order) take one contiguous run
static void check_xcd_run(int total) {
    std::vector<int> seen(total, 0);
    for (int bid = 0; bid < total; ++bid) {
        const int t = nd_xcd_run(bid, total);
        EXPECT(t >= 0 && t < total, "total=%d bid=%d -> %d", total, bid, t);
        if (t >= 0 && t < total) ++seen[t];
        if (bid >= 8) EXPECT(t == nd_xcd_run(bid - 8, total) + 1, "total=%d bid=%d: the run of XCD %d breaks", total, bid, bid % 8);
    }
    for (int t = 0; t < total; ++t) EXPECT(seen[t] == 1, "total=%d: item %d taken %d times", total, t, seen[t]);
}

// every whole tile once (slab -1), every (remainder tile, slab) once, rem_index = tile - n_full
static void check_decode(int n_full, int rem, int split) {
    std::vector<int> whole(n_full, 0), slabs((size_t)rem * split, 0);
    for (int bid = 0; bid < n_full + rem * split; ++bid) {
        const NdTile tl = nd_tile_decode(bid, n_full, split);
        if (bid < n_full) {
            EXPECT(tl.slab == -1 && tl.rem_index == 0 && tl.tile >= 0 && tl.tile < n_full, "n_full=%d bid=%d -> tile %d slab %d", n_full, bid, tl.tile, tl.slab);
            EXPECT(tl.tile == nd_xcd_run(bid, n_full), "n_full=%d bid=%d: whole tiles are not dealt in XCD runs", n_full, bid);
            if (tl.tile >= 0 && tl.tile < n_full) ++whole[tl.tile];
        } else {
            const bool ok = tl.rem_index >= 0 && tl.rem_index < rem && tl.slab >= 0 && tl.slab < split && tl.tile == n_full + tl.rem_index;
            EXPECT(ok, "n_full=%d rem=%d split=%d bid=%d -> tile %d slab %d rem_index %d", n_full, rem, split, bid, tl.tile, tl.slab, tl.rem_index);
            if (ok) ++slabs[(size_t)tl.rem_index * split + tl.slab];
        }
    }
    for (int t = 0; t < n_full; ++t) EXPECT(whole[t] == 1, "n_full=%d: whole tile %d taken %d times", n_full, t, whole[t]);
    for (size_t s = 0; s < slabs.size(); ++s) EXPECT(slabs[s] == 1, "n_full=%d rem=%d split=%d: slab %zu taken %d times", n_full, rem, split, s, slabs[s]);
}

// the slab ranges of a tile partition [0, nk); slab -1 is the whole range
static void check_slabs(int nk, int split) {
    EXPECT(nd_slab_begin(-1, nk, split) == 0 && nd_slab_end(-1, nk, split) == nk, "nk=%d split=%d: whole tile", nk, split);
    int at = 0;
    for (int s = 0; s < split; ++s) {
        const int b = nd_slab_begin(s, nk, split), e = nd_slab_end(s, nk, split);
        EXPECT(b == at && e >= b && e <= nk, "nk=%d split=%d slab %d: [%d, %d) after %d", nk, split, s, b, e, at);
        at = e;
    }
    EXPECT(at == nk, "nk=%d split=%d: the slabs end at %d", nk, split, at);
}

int main() {
    for (int total = 1; total <= 1024; ++total) check_xcd_run(total);
    const int n_fulls[] = {0, 1, 7, 8, 9, 255, 256, 257, 768}, rems[] = {0, 1, 76, 255}, splits[] = {1, 2, 3, 8}, nks[] = {8, 24, 96, 128};
    for (int n_full : n_fulls)
        for (int rem : rems)
            for (int split : splits) check_decode(n_full, rem, split);
    for (int nk : nks)
        for (int split : splits) check_slabs(nk, split);
    printf("%d failed\n", g_failed);
    return g_failed != 0;
}
