"""What the EMA shadow of a noise estimator costs at the config's dimensions (data_dim 150528, hidden_dim = feature_dim = 4096, 2 classes,
1000 timesteps, batches of 30), on one box, in alternating rounds:

    adam        the optimizer pass over encoder_x.0.weight (4096 x 150528 fp32, 2.47 GB) with nd_clip_adam: 7 four-byte streams per parameter
    fused       the same pass with nd_clip_adam_ema: 9 streams (the shadow read and written in the same pass)
    separate    nd_clip_adam followed by the shadow update as two torch launches (mul_, add_): 7 + 2 + 3 = 12 streams
    step        a whole NoiseEstimatorTrainer.step without and with the shadow (the same trainer, its shadow taken away and put back)

    python tools/bench_ema.py [--out profiles/ema_bench.json] [--rounds 5] [--iters 10] [--step_iters 5] [--dims D H F]

Every window is timed with device events around `iters` back-to-back calls after a warm-up of each variant; a round times every variant
once, in turn, so that a drift of the box lands on all of them; the figure of a variant is the median over the rounds, and the spread
(max - min) / median is recorded beside it.  The fused pass is compared with 9/7 of the adam pass OF THE SAME RUN (the bytes it has to
move): fused_over_nine_sevenths; above 1.10 wants an explanation in DESIGN 5.3.  Nothing is gated: exit 0 unless a result is not finite.
Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nested_diffusion_amd import ops                                              # noqa: E402
from nested_diffusion_amd.train_diffusion import NoiseEstimatorTrainer           # noqa: E402

KEY = "encoder_x.0.weight"


def timed(fn, iters: int) -> float:
    """milliseconds per call of `iters` back-to-back calls, by device events"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def summary(rounds):
    med = statistics.median(rounds)
    return round(med, 4), round((max(rounds) - min(rounds)) / med, 4)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10, help="optimizer passes per timed window")
    ap.add_argument("--step_iters", type=int, default=5, help="training steps per timed window")
    ap.add_argument("--dims", type=int, nargs=3, default=(150528, 4096, 4096), metavar=("D", "H", "F"))
    ap.add_argument("--mu", type=float, default=0.9999)
    args = ap.parse_args()
    D, H, F = args.dims
    C, T, B = 2, 1000, 30
    ns = argparse.Namespace
    cfg = ns(data=ns(num_classes=C), model=ns(data_dim=D, hidden_dim=H, feature_dim=F, arch="linear"),
             diffusion=ns(timesteps=T, beta_schedule="linear", beta_start=1e-4, beta_end=0.02, include_guidance=True),
             optim=ns(optimizer="Adam", lr=1e-3, beta1=0.9, eps=1e-8, weight_decay=0.0, amsgrad=False, grad_clip=1.0))
    dev = torch.device("cuda")
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    trainer = NoiseEstimatorTrainer(cfg, dev, seed=0, ema_rate=args.mu)
    torch.cuda.synchronize()
    shadow_bytes = sum((q.data if isinstance(q, ops.PackedWeight) else q).numel() * 4 for q in trainer.shadow.values())
    resident = torch.cuda.memory_allocated() - base
    plain_bytes = resident - shadow_bytes
    print(f"trainer at D={D} H={H} F={F}: {resident / 1e9:.2f} GB resident, {shadow_bytes / 1e9:.2f} GB of it the shadow", flush=True)

    # ---- the optimizer pass over the largest weight, on the trainer's own images ------------------------------------------------------------
    w, m, v, s = trainer.p[KEY], trainer.m[KEY], trainer.v[KEY], trainer.shadow[KEY]
    g = w.zeros_like()
    g.data.normal_(0.0, 1e-3, generator=torch.Generator(device=dev).manual_seed(1))
    n = w.data.numel()
    sumsq = ops.sumsq(g)
    a, e = ops.adam_step(1e-3, 10), ops.ema_step(args.mu)
    mu32, om32 = float(e.mu), float(e.one_minus_mu)

    def p_adam():
        ops.clip_adam(w, m, v, g, a, sumsq=sumsq, max_norm=1.0)

    def p_fused():
        ops.clip_adam(w, m, v, g, a, sumsq=sumsq, max_norm=1.0, shadow=s, ema=e)

    def p_separate():
        ops.clip_adam(w, m, v, g, a, sumsq=sumsq, max_norm=1.0)
        s.data.mul_(mu32).add_(w.data, alpha=om32)

    passes = {"adam": p_adam, "fused": p_fused, "separate": p_separate}
    for fn in passes.values():                                                    # warm-up: code objects, the allocator
        timed(fn, 2)
    pass_ms = {k: [] for k in passes}
    for r in range(args.rounds):
        for k, fn in passes.items():
            pass_ms[k].append(timed(fn, args.iters))
        print(f"round {r}: " + ", ".join(f"{k} {pass_ms[k][-1]:.3f} ms" for k in passes), flush=True)
    del g

    # ---- a whole step, the shadow taken away and put back ---------------------------------------------------------------------------------------
    gen = torch.Generator(device=dev).manual_seed(2)
    x = torch.rand(B, D, generator=gen, device=dev)
    y0 = torch.nn.functional.one_hot(torch.arange(B) % C, C).float().to(dev)
    yhat = torch.softmax(torch.randn(B, C, generator=gen, device=dev), dim=1)
    e_noise = torch.randn(B, C, generator=gen, device=dev)
    t = (torch.arange(B, dtype=torch.int64) * 37) % T
    shadow = trainer.shadow

    def step_with(sh):
        def run():
            trainer.shadow = sh
            trainer.step(x, y0, yhat, t, e_noise)
        return run

    steps = {"plain": step_with(None), "ema": step_with(shadow)}
    for fn in steps.values():
        timed(fn, 2)
    step_ms = {k: [] for k in steps}
    for r in range(args.rounds):
        for k, fn in steps.items():
            step_ms[k].append(timed(fn, args.step_iters))
        print(f"round {r}: " + ", ".join(f"step {k} {step_ms[k][-1]:.3f} ms" for k in steps), flush=True)
    trainer.shadow = shadow

    adam, adam_spread = summary(pass_ms["adam"])
    fused, fused_spread = summary(pass_ms["fused"])
    sep, sep_spread = summary(pass_ms["separate"])
    sp, sp_spread = summary(step_ms["plain"])
    se, se_spread = summary(step_ms["ema"])
    res = {"what": "EMA shadow in the clip + Adam pass", "data_dim": D, "hidden_dim": H, "feature_dim": F, "batch": B, "mu": args.mu,
           "pass_floats": n, "rounds": args.rounds, "iters": args.iters, "step_iters": args.step_iters,
           "pass_adam_ms": adam, "pass_adam_spread": adam_spread, "pass_fused_ms": fused, "pass_fused_spread": fused_spread,
           "pass_separate_ms": sep, "pass_separate_spread": sep_spread,
           "pass_adam_tb_s": round(7 * 4 * n / (adam * 1e-3) / 1e12, 3), "pass_fused_tb_s": round(9 * 4 * n / (fused * 1e-3) / 1e12, 3),
           "fused_over_adam": round(fused / adam, 4), "fused_over_nine_sevenths": round(fused / (adam * 9.0 / 7.0), 4),
           "separate_over_fused": round(sep / fused, 4),
           "step_plain_ms": sp, "step_plain_spread": sp_spread, "step_ema_ms": se, "step_ema_spread": se_spread,
           "step_ema_over_plain": round(se / sp, 4), "step_extra_ms": round(se - sp, 3),
           "shadow_gb": round(shadow_bytes / 1e9, 3), "resident_without_shadow_gb": round(plain_bytes / 1e9, 3),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    finite = all(x == x and x != float("inf") for x in (adam, fused, sep, sp, se))
    return 0 if finite else 1


if __name__ == "__main__":
    sys.exit(main())
