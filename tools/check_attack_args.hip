// check_attack_args.hip -- the refusals of the attack entry points (nd_attack_linf.hip, nd_attack_l2.hip, nd_apgd_l2.hip, nd_square.hip) as a stand-alone
// host program: every call below returns ND_ERR_ARG before any HIP call, so it needs no GPU.  Meant for a host-side sanitizer build
// (CPU only, never on a GPU box); the device pass is left alone:
//   cd nested_diffusion_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-gpu-sanitize \
//       ../../tools/check_attack_args.hip nd_error.hip nd_attack_linf.hip nd_attack_l2.hip nd_apgd_l2.hip nd_square.hip -o ../../tools/bin/check_attack_args
//   ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=halt_on_error=1 ../../tools/bin/check_attack_args
#include <stdio.h>
#include <string.h>
#include "../nested_diffusion_amd/csrc/nd_host.hpp"

static int g_failed = 0;

static void expect(int rc, const char* want, const char* call) {
    const bool ok = rc == ND_ERR_ARG && strstr(nd_last_error(), want);
    printf("%s  %-28s rc=%d  \"%s\"\n", ok ? "ok  " : "FAIL", call, rc, nd_last_error());
    g_failed += !ok;
    nd_set_err(ND_OK, "%s", "");
}

int main() {
    float* P = (float*)4096;                        // a non-NULL, 16-byte aligned address, never dereferenced
    float* Q = (float*)4100;                        // misaligned
    int64_t* I = (int64_t*)4096;
    int32_t* J = (int32_t*)4096;
    uint32_t* U = (uint32_t*)4096;
    const size_t q31 = (size_t)0x7FFFFFFF * 4;      // per_image / 4 == 0x7FFFFFFF: APGD takes it, L2 does not

    expect(nd_linf_step(nullptr, P, P, P, 8, .1f, .1f, 0, 1, nullptr), "NULL tensor", "linf_step NULL");
    expect(nd_linf_random_start(P, nullptr, 2, 8, 1, 0, 0, .1f, 0, 1, nullptr), "NULL tensor", "linf_start NULL");
    expect(nd_linf_random_start(P, P, 2, 6, 1, 0, 0, .1f, 0, 1, nullptr), "random start needs", "linf_start per_image=6");
    expect(nd_linf_random_start(P, P, 0, 8, 1, 0, 0, .1f, 0, 1, nullptr), "per_image % 4 == 0 (B=0, per_image=8)", "linf_start B=0");
    expect(nd_linf_random_start(P, P, 70000, 0, 1, 0, 0, .1f, 0, 1, nullptr), "per_image=0", "linf_start per_image=0");
    expect(nd_linf_random_start(P, P, 2, q31 + 4, 1, 0, 0, .1f, 0, 1, nullptr), "random start needs", "linf_start quads=2^31");

    expect(nd_apgd_random_start(P, nullptr, P, U, 2, 8, 1, 0, .1f, 0, 1, nullptr), "NULL tensor", "apgd_start NULL");
    expect(nd_apgd_random_start(P, I, P, U, 2, 6, 1, 0, .1f, 0, 1, nullptr), "apgd random start needs 1 <= B <= 65535 and per_image % 4 == 0", "apgd_start per_image=6");
    expect(nd_apgd_random_start(P, I, P, U, 0, 8, 1, 0, .1f, 0, 1, nullptr), "1 <= B <= 65535", "apgd_start B=0");
    expect(nd_apgd_random_start(P, I, P, U, 65536, 8, 1, 0, .1f, 0, 1, nullptr), "1 <= B <= 65535", "apgd_start B=65536");
    expect(nd_apgd_random_start(P, I, P, U, 2, q31 + 4, 1, 0, .1f, 0, 1, nullptr), "apgd random start needs 1 <= B", "apgd_start quads=2^31");
    expect(nd_apgd_random_start(Q, I, P, U, 2, q31, 1, 0, .1f, 0, 1, nullptr), "16-byte aligned", "apgd_start quads=2^31-1");
    expect(nd_apgd_random_start(P, I, Q, U, 2, 8, 1, 0, .1f, 0, 1, nullptr), "16-byte aligned", "apgd_start misaligned out");

    expect(nd_apgd_control(P, I, P, P, P, P, J, J, P, nullptr, 2, 2, 100, 5, 0, .75f, 0, nullptr), "NULL tensor", "apgd_control NULL");
    expect(nd_apgd_control(P, I, P, P, P, P, J, J, P, J, 2, 1025, 100, 0, 0, .75f, 0, nullptr), "C <= 1024 (C=1025)", "apgd_control C=1025");
    expect(nd_apgd_control(P, I, P, P, P, P, J, J, P, J, 2, 2, 100, 100, 0, .75f, 0, nullptr), "iter < n_iter", "apgd_control iter=n_iter");
    expect(nd_apgd_control(P, I, P, P, P, P, J, J, P, J, 2, 2, 100, 5, 7, .75f, 0, nullptr), "(iter=5, k=7", "apgd_control k=7");

    expect(nd_apgd_update(P, nullptr, P, P, P, P, P, J, P, 2, 8, .1f, .75f, 1, nullptr), "NULL tensor", "apgd_update NULL");
    expect(nd_apgd_update(P, P, P, P, nullptr, P, P, J, P, 2, 8, .1f, .75f, 1, nullptr), "with flags needs", "apgd_update no x_best");
    expect(nd_apgd_update(P, P, nullptr, P, nullptr, nullptr, nullptr, nullptr, P, 2, 8, .1f, 1, 1, nullptr), "with a step needs", "apgd_update no x_adv_old");
    expect(nd_apgd_update(P, P, P, P, P, P, P, J, P, 2, 6, .1f, .75f, 1, nullptr), "apgd update needs 1 <= B <= 65535 and per_image % 4 == 0", "apgd_update per_image=6");
    expect(nd_apgd_update(P, P, P, P, P, P, P, J, P, 65536, 8, .1f, .75f, 1, nullptr), "1 <= B <= 65535", "apgd_update B=65536");
    expect(nd_apgd_update(P, P, P, P, P, P, Q, J, P, 2, q31, .1f, .75f, 1, nullptr), "16-byte aligned", "apgd_update quads=2^31-1");

    expect(nd_l2_step(P, P, P, P, nullptr, P, P, 2, 8, .1f, 1, 0, 1, nullptr), "NULL tensor", "l2_step NULL");
    expect(nd_l2_step(P, P, P, P, P, P, P, 2, 6, .1f, 1, 0, 1, nullptr), "l2 step needs 1 <= B <= 65535 and per_image % 4 == 0 (B=2, per_image=6)", "l2_step per_image=6");
    expect(nd_l2_step(Q, P, P, P, P, P, P, 2, q31, .1f, 1, 0, 1, nullptr), "l2 step needs 1 <= B", "l2_step quads=2^31-1");
    expect(nd_l2_step(P, P, Q, P, P, P, P, 2, 8, .1f, 1, 0, 1, nullptr), "l2 step needs 16-byte aligned", "l2_step misaligned grad");
    expect(nd_l2_random_start(P, P, P, P, 65536, 8, 1, 0, 0, 1, 0, 1, nullptr), "l2 random start needs 1 <= B <= 65535", "l2_start B=65536");
    expect(nd_l2_random_start(P, Q, P, P, 2, 8, 1, 0, 0, 1, 0, 1, nullptr), "l2 random start needs 16-byte aligned", "l2_start misaligned out");
    expect(nd_cw_attack_space(P, P, P, 6, 0, 1, nullptr), "n % 4 == 0", "cw_attack_space n=6");
    expect(nd_cw_attack_space(P, P, Q, 8, 0, 1, nullptr), "cw attack space needs 16-byte aligned", "cw_attack_space misaligned");
    expect(nd_cw_model_space(P, P, P, P, P, P, P, P, P, 2, 0, 0, 1, nullptr), "cw model space needs 1 <= B", "cw_model_space per_image=0");
    expect(nd_cw_model_space(P, P, P, P, P, Q, P, P, P, 2, 8, 0, 1, nullptr), "cw model space needs 16-byte aligned", "cw_model_space misaligned");
    expect(nd_cw_control(P, I, P, P, P, P, P, J, J, P, 65536, 2, 0, nullptr), "1 <= B <= 65535", "cw_control B=65536");
    expect(nd_cw_update(P, P, P, P, P, P, P, P, J, 0, 8, .01f, .1f, .001f, .5f, nullptr), "cw update needs 1 <= B", "cw_update B=0");
    expect(nd_cw_update(P, P, P, P, P, P, P, Q, J, 2, 8, .01f, .1f, .001f, .5f, nullptr), "cw update needs 16-byte aligned", "cw_update misaligned best");

    expect(nd_apgd_l2_random_start(P, I, nullptr, P, P, 2, 8, 1, 0, .5f, 0, 1, nullptr), "nd_apgd_l2_random_start: NULL", "apgd_l2_start NULL out");
    expect(nd_apgd_l2_random_start(P, I, P, P, P, 0, 8, 1, 0, .5f, 0, 1, nullptr), "nd_apgd_l2_random_start needs 1 <= B <= 65535", "apgd_l2_start B=0");
    expect(nd_apgd_l2_random_start(P, I, P, P, P, 2, 6, 1, 0, .5f, 0, 1, nullptr), "per_image % 4 == 0 (B=2, per_image=6)", "apgd_l2_start per_image=6");
    expect(nd_apgd_l2_random_start(P, I, P, P, P, 2, q31, 1, 0, .5f, 0, 1, nullptr), "nd_apgd_l2_random_start needs 1 <= B", "apgd_l2_start quads=2^31-1");
    expect(nd_apgd_l2_random_start(P, I, Q, P, P, 2, 8, 1, 0, .5f, 0, 1, nullptr), "nd_apgd_l2_random_start needs 16-byte aligned", "apgd_l2_start misaligned out");
    expect(nd_apgd_l2_step(nullptr, P, P, P, nullptr, nullptr, P, P, P, 2, 8, .5f, 1.f, nullptr), "nd_apgd_l2_step: NULL", "apgd_l2_step NULL x");
    expect(nd_apgd_l2_step(P, P, P, P, nullptr, J, P, P, P, 2, 8, .5f, .75f, nullptr), "with flags needs grad_best", "apgd_l2_step flags, no grad_best");
    expect(nd_apgd_l2_step(P, P, P, P, P, J, P, P, P, 65536, 8, .5f, .75f, nullptr), "nd_apgd_l2_step needs 1 <= B <= 65535", "apgd_l2_step B=65536");
    expect(nd_apgd_l2_step(P, P, P, P, P, J, P, P, P, 2, 10, .5f, .75f, nullptr), "per_image % 4 == 0 (B=2, per_image=10)", "apgd_l2_step per_image=10");
    expect(nd_apgd_l2_step(P, P, P, P, Q, J, P, P, P, 2, 8, .5f, .75f, nullptr), "nd_apgd_l2_step needs 16-byte aligned", "apgd_l2_step misaligned grad_best");
    expect(nd_eot_add(nullptr, P, 8, 0, nullptr), "nd_eot_add: NULL", "eot_add NULL acc");
    expect(nd_eot_add(P, P, 6, 0, nullptr), "n % 4 == 0", "eot_add n=6");
    expect(nd_eot_add(P, P, 8, -1, nullptr), "divisor >= 0", "eot_add divisor=-1");
    expect(nd_eot_add(P, Q, 8, 2, nullptr), "nd_eot_add needs 16-byte aligned", "eot_add misaligned g");

    expect(nd_square_init(P, nullptr, P, P, 2, 3, 8, 8, 1, 0, .1f, 0, 1, nullptr), "NULL tensor", "square_init NULL");
    expect(nd_square_init(P, I, P, P, 65536, 3, 8, 8, 1, 0, .1f, 0, 1, nullptr), "(B=65536)", "square_init B=65536");
    expect(nd_square_propose(P, P, P, I, P, J, 2, 33, 8, 8, 2, 0, 1, 0, .1f, 0, 1, nullptr), "1 <= Cin <= 32", "square_propose Cin=33");
    expect(nd_square_propose(P, P, P, I, P, J, 2, 3, 12, 8, 9, 0, 1, 0, .1f, 0, 1, nullptr), "1 <= s <= min(H, W)", "square_propose s=9");
    expect(nd_square_accept(P, I, P, P, J, J, 2, 1, 0, nullptr), "2 <= C <= 1024", "square_accept C=1");
    expect(nd_square_commit(P, P, J, J, 2, 3, 4097, 8, 2, nullptr), "1 <= H, W <= 4096", "square_commit H=4097");

    // the shared grid helper: nd_l2_parts is its only exported face
    const size_t per[] = {0, 4, 1024, 1028, 3072, 150528, 4 * 256 * 256, 4 * 256 * 300, q31};
    const int want[] = {1, 1, 1, 2, 3, 147, 256, 256, 256};
    for (int i = 0; i < 9; ++i) {
        const int got = nd_l2_parts(per[i]);
        printf("%s  nd_l2_parts(%zu) = %d\n", got == want[i] ? "ok  " : "FAIL", per[i], got);
        g_failed += got != want[i];
    }
    printf("%d failed\n", g_failed);
    return g_failed != 0;
}
