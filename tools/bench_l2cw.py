"""Cost of the L2 attacks' and Carlini & Wagner's passes at the shape of an attacked evaluation: B = 32, ViT-B/16, 224 x 224.

    python tools/bench_l2cw.py [--batch 32] [--reps 5]

Prints one JSON line: ms per input_grad and per input_grad_margin (alternating runs), per nd_l2_step and nd_l2_random_start, per L2 BIM
iteration (input_grad + nd_l2_step) and BIM batch (10 iterations), the elementwise passes of one CW iteration alone (nd_cw_model_space +
nd_cw_control + nd_cw_update), one whole CW iteration, and one binary-search step of 20 iterations (abort_early off: no read-back inside).
Warm-up first, medians over --reps; the small passes are timed 20 at a time.  bytes_* are the algorithmic bytes of a pass
(4 B x B x 150528 elements x arrays read or written), for a rate against the HBM peak.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from nested_diffusion_amd import ops
    from nested_diffusion_amd.attack import CarliniWagner, L2Attack
    from nested_diffusion_amd.mapping import VisionTransformer
    from oracle import ref_cpu
    assert torch.cuda.is_available(), "bench_l2cw needs the GPU"
    B, dev = a.batch, "cuda"
    vit = VisionTransformer(ref_cpu.init_vit_params(embed=768, depth=12, img=224, seed=1), 12, dev)
    g = torch.Generator().manual_seed(2)
    x0 = torch.rand(B, 3, 224, 224, generator=g).to(dev)
    y = vit.forward(x0).argmax(1)
    consts = torch.full((B,), 10.0, device=dev)
    grad = lambda: vit.input_grad(x0, y)                                       # noqa: E731
    mgrad = lambda: vit.input_grad_margin(x0, y, consts, check_labels=False)   # noqa: E731
    _, g0, _ = grad()
    x = ops.l2_random_start(x0, 2.0, 0)
    bim = L2Attack(2.0, "BIM", vit)
    w0, xrec = ops.cw_attack_space(x0)
    s = ops.CwState(x0)
    logits, dx, margin = mgrad()

    def cw_passes():
        ops.cw_model_space(w0, x0, xrec, s)
        ops.cw_control(logits, y, consts, margin, s)
        ops.cw_update(s, dx, xrec, 0.01, 3)

    def cw_iter():
        xx = ops.cw_model_space(w0, x0, xrec, s)
        lg, d, m = vit.input_grad_margin(xx, y, consts, check_labels=False)
        ops.cw_control(lg, y, consts, m, s)
        ops.cw_update(s, d, xrec, 0.01, 3)

    step = lambda: ops.l2_step(x, x0, g0, 0.4, 2.0)                            # noqa: E731
    start = lambda: ops.l2_random_start(x0, 2.0, 0)                            # noqa: E731
    cw = CarliniWagner(4.0, vit, binary_search_steps=1, steps=20, abort_early=False)
    for f in (grad, mgrad, step, start, cw_passes, cw_iter, lambda: bim.step(x, x0, y)):
        f()
    tg, tm = [], []
    for _ in range(a.reps):
        tg += timed(grad, 1)
        tm += timed(mgrad, 1)
    many = lambda f: [t / 20 for t in timed(lambda: [f() for _ in range(20)], a.reps)]   # noqa: E731
    t_step, t_start, t_pass = many(step), many(start), many(cw_passes)
    t_bim_iter = timed(lambda: bim.step(x, x0, y), a.reps)
    t_bim = timed(lambda: bim.generate_attack(x0, y), max(1, a.reps // 2))
    t_cw_iter = timed(cw_iter, a.reps)
    t_cw_bs = timed(lambda: cw.generate_attack(x0, y), max(1, a.reps // 2))
    med = statistics.median
    n = 4.0 * B * 150528
    r = {"tool": "bench_l2cw", "batch": B, "model": "vit_base_patch16_224", "input_grad_ms": med(tg), "input_grad_margin_ms": med(tm),
         "l2_step_ms": med(t_step), "l2_step_gbps": 8 * n / med(t_step) / 1e6, "l2_random_start_ms": med(t_start),
         "bim_iter_ms": med(t_bim_iter), "bim_batch_ms": med(t_bim), "l2_step_over_input_grad": med(t_step) / med(tg),
         "cw_passes_ms": med(t_pass), "cw_passes_gbps": 17 * n / med(t_pass) / 1e6, "cw_iter_ms": med(t_cw_iter),
         "cw_passes_over_iter": med(t_pass) / med(t_cw_iter), "cw_search_step_20_ms": med(t_cw_bs),
         "bytes_note": "l2_step: g, then x, g, x0, then x, g, x0, out = 8 arrays; cw passes: w0, delta, xrec, x0 in, t, x out (6), then "
                       "x, xrec, t, dx, delta, m, v in, delta, m, v out, best in flagged rows (11)",
         "device": torch.cuda.get_device_name(0)}
    print(json.dumps(r))


if __name__ == "__main__":
    main()
