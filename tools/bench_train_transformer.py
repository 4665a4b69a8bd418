"""One training step of the ViT at ViT-B/16, batch 30, 224 x 224 synthetic images: the whole ViTTrainer.step, and the fused weight-gradient +
AdamW kernel (nd_gemm_tn_adamw) on each production shape alone, set against the f32-input-MFMA rate.  GPU only.

    python tools/bench_train_transformer.py [--batch 30] [--reps 5] [--rounds 5] [--out FILE]

Prints one JSON line (and writes it to --out): times in ms (median over the rounds, each a window of `reps` calls between two device
events), the kernel's TFLOP/s = 2 M N K / time per shape, the sum of the kernel's time over the layers of a step (shape time x count)
and its share of the step."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nested_diffusion_amd import ops, synthetic  # noqa: E402
from nested_diffusion_amd.train_transformer import ViTTrainer  # noqa: E402

MFMA_F32_PEAK_TFLOPS = 155.0


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def timed(fns, reps, rounds):
    """median ms per call of each function, the functions' windows alternating within a round"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    samples = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            samples[i].append(window(fn, reps))
    return [statistics.median(s) for s in samples], [(min(s), max(s)) for s in samples]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_transformer needs the GPU: there is nothing to measure without one")
    dev, B = "cuda", a.batch
    tr = ViTTrainer(synthetic.vit_state(seed=7, device=dev), num_classes=2, num_heads=12)
    img = synthetic.images(B, device=dev)
    labels = torch.arange(B, device=dev) % 2
    adamw = ops.adamw_step(1e-4, 10)
    M = B * 197
    # (name, M, N, K, launches per step)
    shapes = [("qkv", M, 2304, 768, 12), ("proj", M, 768, 768, 12), ("fc1", M, 3072, 768, 12), ("fc2", M, 768, 3072, 12),
              ("patch_embed", B * 196, 768, 768, 1), ("head", B, 2, 768, 1)]
    bufs = []
    for _, m_, n_, k_, _ in shapes:
        bufs.append((torch.randn(m_, n_, device=dev) * 1e-3, torch.randn(m_, k_, device=dev), torch.randn(n_, k_, device=dev) * 0.02,
                     torch.zeros(n_, k_, device=dev), torch.zeros(n_, k_, device=dev)))
    fns = [lambda: tr.step(img, labels), lambda: tr.vit.forward(img)]
    for dy, x, w, m, v in bufs:
        fns.append(lambda dy=dy, x=x, w=w, m=m, v=v: ops.gemm_tn_adamw(dy, x, w, m, v, adamw, gscale=1.0 / B))
    times, spans = timed(fns, a.reps, a.rounds)
    t_step, t_fwd, t_shapes = times[0], times[1], times[2:]
    flop = sum(2.0 * m_ * n_ * k_ * c for _, m_, n_, k_, c in shapes)
    t_kernel = sum(t * s[4] for t, s in zip(t_shapes, shapes))
    res = {"tool": "bench_train_transformer", "batch": B, "step_ms": round(t_step, 2), "forward_ms": round(t_fwd, 2),
           "gemm_tn_adamw_ms": round(t_kernel, 2), "share_of_step": round(t_kernel / t_step, 3), "wgrad_tflop": round(flop / 1e12, 3),
           "gemm_tn_adamw_tflops": round(flop / t_kernel / 1e9, 1), "fraction_of_mfma_f32_peak": round(flop / t_kernel / 1e9 / MFMA_F32_PEAK_TFLOPS, 3),
           "shapes": {n: {"M": m_, "N": n_, "K": k_, "ms": round(t, 4), "tflops": round(2.0 * m_ * n_ * k_ / t / 1e9, 1)}
                      for t, (n, m_, n_, k_, _) in zip(t_shapes, shapes)},
           "step_ms_min_max": [round(s, 2) for s in spans[0]], "reps": a.reps, "rounds": a.rounds}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
