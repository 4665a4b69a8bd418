"""One training step of a mapping MLP at config dims (ViT-B/16 prefix, 150528 -> 4096 -> 2048 -> 128 -> 2, batch 30): the whole
MappingTrainer.step, and the fused weight-gradient + Adam kernel of linear1 alone against its floor -- 24 bytes per parameter (W, m, v
read and written once) at the 8 TB/s HBM peak.  GPU only.

    python tools/bench_train_mapping.py [--batch 30] [--mn_idx 0] [--reps 20] [--rounds 5] [--out FILE]

Prints one JSON line (and writes it to --out): times in ms (median over the rounds, each a window of `reps` calls between two device
events), the kernel's TB/s = 24 B x parameters / time, its fraction of the floor and its share of the step."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nested_diffusion_amd import ops, synthetic  # noqa: E402
from nested_diffusion_amd.mapping import VisionTransformer  # noqa: E402
from nested_diffusion_amd.train_mapping import MappingTrainer  # noqa: E402

HBM_PEAK_TBPS = 8.0


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
    ap.add_argument("--mn_idx", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_mapping needs the GPU: there is nothing to measure without one")
    dev, B = "cuda", a.batch
    vit = VisionTransformer(synthetic.vit_state(seed=7, device=dev), 12, dev)
    tr = MappingTrainer(vit, a.mn_idx, num_classes=2, lr=1e-3, seed=0)
    img = synthetic.images(B, device=dev)
    labels = torch.arange(B, device=dev) % 2
    w, m, v = tr.model.p["linear1.weight"], tr.m["linear1.weight"], tr.v["linear1.weight"]
    x1 = torch.randn(B, w.K, device=dev)
    dy1 = torch.randn(B, w.N, device=dev) * 1e-3
    b1 = tr.model.p["linear1.bias"]
    adam = ops.adam_step(1e-3, 10)
    fns = [lambda: tr.step(img, labels),
           lambda: ops.linear_wgrad_adam(dy1, x1, w, m, v, adam, gscale=1.0 / B),
           lambda: ops.linear(x1, w, b1, act="relu"),
           lambda: tr.features(img)]
    (t_step, t_wg, t_fwd, t_prefix), spans = timed(fns, a.reps, a.rounds)
    params = w.N * w.K
    traffic = 24.0 * params
    floor_ms = traffic / (HBM_PEAK_TBPS * 1e12) * 1e3
    res = {"tool": "bench_train_mapping", "batch": B, "mn_idx": a.mn_idx, "layer1": [w.K, w.N], "traffic_gb": round(traffic / 1e9, 3),
           "step_ms": round(t_step, 3), "wgrad_adam_l1_ms": round(t_wg, 4), "wgrad_adam_l1_tbps": round(traffic / t_wg / 1e9, 3),
           "floor_ms": round(floor_ms, 4), "fraction_of_floor": round(floor_ms / t_wg, 3), "share_of_step": round(t_wg / t_step, 3),
           "linear1_fwd_ms": round(t_fwd, 4), "prefix_ms": round(t_prefix, 3),
           "step_ms_min_max": [round(s, 3) for s in spans[0]], "wgrad_adam_l1_ms_min_max": [round(s, 4) for s in spans[1]],
           "reps": a.reps, "rounds": a.rounds}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
