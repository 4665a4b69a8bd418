"""Cost of APGD-L2's step beside what an iteration costs, at the shape of an attacked evaluation: B = 32, ViT-B/16, 224 x 224.

    python tools/bench_apgd_l2.py [--batch 32] [--reps 7]

Prints one JSON line: us per nd_apgd_l2_step (with flags: the step of an iteration after the first), per nd_apgd_update (Linf: the flags'
copies and the momentum step in one pass, the same shape), per nd_apgd_update without a step (what the L2 iteration runs in front of its
step), per nd_eot_add; ms per ViT-B input_grad and per whole L2 iteration (input_grad, nd_apgd_control, nd_apgd_update without a step,
nd_apgd_l2_step), and the step's share of that iteration.  Warm-up first, medians over --reps; the small passes are timed 20 at a time.
bytes_step is the algorithmic traffic of the step's four launches: g (1 array), then xa, g, x (3), then xa, x_adv_old, g, x (4), then
the same four read and two written (6) = 14 arrays of 4 B x B x 150528, for a rate against the HBM peak.
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
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    from nested_diffusion_amd import ops
    from nested_diffusion_amd.mapping import VisionTransformer
    from oracle import ref_cpu
    assert torch.cuda.is_available(), "bench_apgd_l2 needs the GPU"
    B, dev, eps, n_iter = a.batch, "cuda", 2.0, 100
    vit = VisionTransformer(ref_cpu.init_vit_params(embed=768, depth=12, img=224, seed=1), 12, dev)
    x = torch.rand(B, 3, 224, 224, generator=torch.Generator().manual_seed(2)).to(dev)
    y = vit.forward(x).argmax(1)
    index = torch.arange(B, device=dev)
    x_adv = ops.apgd_l2_random_start(x, index, eps, 0)
    logits, grad, loss = vit.input_grad(x_adv, y)
    st = ops.ApgdState(B, n_iter, dev)
    ops.apgd_control(logits, y, loss, st, -1, 0, step0=2.0 * eps)
    x_best, x_best_adv, grad_best, x_adv_old = x_adv.clone(), x_adv.clone(), grad.clone(), x_adv.clone()
    flags = torch.tensor([k % 8 for k in range(B)], dtype=torch.int32, device=dev)     # every flag value, RESTORE in half of the rows

    l2_step = lambda: ops.apgd_l2_step(x, x_adv, x_adv_old, grad, grad_best, flags, st.step, eps, 0.75)                        # noqa: E731
    linf_update = lambda: ops.apgd_update(x, x_adv, x_adv_old, grad, x_best, grad_best, x_best_adv, flags, st.step, 8 / 255, 0.75, True)   # noqa: E731
    copies = lambda: ops.apgd_update(None, x_adv, None, grad, x_best, grad_best, x_best_adv, flags, None, eps, 0.75, False)    # noqa: E731
    eot = lambda: ops.eot_add(grad_best, grad, 2)                                                                             # noqa: E731
    in_grad = lambda: vit.input_grad(x_adv, y)                                                                                # noqa: E731

    def l2_iter():
        lg, g, ls = vit.input_grad(x_adv, y)
        f = ops.apgd_control(lg, y, ls, st, 3, 0)
        ops.apgd_update(None, x_adv, None, g, x_best, grad_best, x_best_adv, f, None, eps, 0.75, False)
        ops.apgd_l2_step(x, x_adv, x_adv_old, g, grad_best, f, st.step, eps, 0.75)

    for f in (l2_step, linf_update, copies, eot, in_grad, l2_iter):
        f()
    many = lambda f: [t / 20 for t in timed(lambda: [f() for _ in range(20)], a.reps)]   # noqa: E731
    t_step, t_linf, t_copies, t_eot = many(l2_step), many(linf_update), many(copies), many(eot)
    t_grad, t_iter = timed(in_grad, a.reps), timed(l2_iter, a.reps)
    med = statistics.median
    n = 4.0 * B * 150528
    r = {"tool": "bench_apgd_l2", "batch": B, "model": "vit_base_patch16_224", "apgd_l2_step_us": med(t_step) * 1e3,
         "apgd_l2_step_gbps": 14 * n / med(t_step) / 1e6, "apgd_update_linf_us": med(t_linf) * 1e3, "apgd_update_copies_us": med(t_copies) * 1e3,
         "eot_add_us": med(t_eot) * 1e3, "input_grad_ms": med(t_grad), "l2_iter_ms": med(t_iter),
         "step_share_of_iter_percent": 100.0 * med(t_step) / med(t_iter), "step_over_input_grad_percent": 100.0 * med(t_step) / med(t_grad),
         "step_over_linf_update": med(t_step) / med(t_linf), "bytes_step": 14 * n, "reps": a.reps,
         "device": torch.cuda.get_device_name(0)}
    print(json.dumps(r))


if __name__ == "__main__":
    main()
