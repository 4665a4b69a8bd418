"""What a sampler plan (main --sample_steps: S of the schedule's T timesteps per chain) buys and what it changes, at the config's own shape.

    python tools/bench_strided_sampler.py [--K 5] [--T 1000] [--B 32] [--mc 1] [--steps 100,50,20,10] [--grad_steps 100,10]
                                          [--warmup 2] [--repeat 5] [--bench_this FILE ...] [--bench_parent FILE ...] [--out FILE]

Synthetic weights of the reference's shapes (ViT-B/16, five mapping MLPs, K denoiser-structured noise estimators with D = 150528,
H = F = 4096, embedding tables of T rows), fp32, one GPU.  Writes ONE JSON line (default: profiles/strided_sampler.json):

  predict_batch   per "full" (no plan: all T timesteps) and "S<n>_eta<0|1>" (uniform sequence): ms = the median of `repeat` calls of
                  Diffusion.predict_batch after `warmup` (device-synchronised, host-timed: one hipGraph launch per call), the steps that
                  ran, and against the FULL chain on the same images: max_prob_diff = the largest difference of the ensemble's class
                  probabilities over the batch, equal_votes = the share of images with the same majority vote.  The noise is explicit:
                  one tensor [K, T, B mc, C]; a chain of S steps reads its first S rows (row 0, the start y_T, is shared; at eta = 0
                  nothing else is read).  These are REPORTED: a member with other weights moves them, nothing here asserts a bound.
  input_grad      per "S<n>": ms per EnsembleTarget.input_grad (sample_steps = n, eta = 1, fresh noise per call), same timing rule.
  default_path    the `value` of bench.py runs of this tree and of its parent commit on the same machine (--bench_this / --bench_parent:
                  files holding bench.py's JSON line), side by side: a run without a plan must not pay for the feature."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def median_ms(fn, warmup, repeat):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def bench_values(paths):
    out = []
    for p in paths or ():
        line = [l for l in open(p).read().splitlines() if l.strip().startswith("{")][-1]
        out.append(float(json.loads(line)["value"]))
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=5)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--mc", type=int, default=1)
    ap.add_argument("--steps", type=str, default="100,50,20,10")
    ap.add_argument("--grad_steps", type=str, default="100,10")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--bench_this", type=str, nargs="*", default=[])
    ap.add_argument("--bench_parent", type=str, nargs="*", default=[])
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "strided_sampler.json"))
    a = ap.parse_args(argv)
    from nested_diffusion_amd import synthetic
    from nested_diffusion_amd.ensemble_grad import EnsembleTarget
    from nested_diffusion_amd.mapping import Classifier, GuidingConditioner, VisionTransformer
    from nested_diffusion_amd.runner import Diffusion
    ns = types.SimpleNamespace
    dev, C, D, H, F = "cuda", 2, 150528, 4096, 4096
    cfg = ns(data=ns(dataset="ChestXRay", num_classes=C), model=ns(data_dim=D, hidden_dim=H, feature_dim=F, arch="linear"),
             diffusion=ns(timesteps=a.T, beta_schedule="linear", beta_start=1e-4, beta_end=0.02, aux_cls=ns(arch="sevit"),
                          trained_aux_cls_ckpt_path="", trained_diffusion_ckpt_path=[[]], include_guidance=True),
             testing=ns(batch_size=a.B))
    cond = GuidingConditioner(VisionTransformer(synthetic.vit_state(1, device=dev), 12, dev),
                              [Classifier(synthetic.classifier_state(196 * 768, 10 + k, device=dev), dev) for k in range(a.K)])
    states = [synthetic.cond_model_state(D, H, F, C, a.T, 40 + k, device=dev, denoiser=True) for k in range(a.K)]
    x = synthetic.images(a.B, device=dev)
    labels = torch.arange(a.B, device=dev) % C
    r = {"shape": dict(K=a.K, T=a.T, B=a.B, mc=a.mc, D=D, H=H, F=F, dtype="f32", members="denoiser-structured", skip_type="uniform"),
         "warmup": a.warmup, "repeat": a.repeat, "predict_batch": {}, "input_grad": {}}

    # the adaptive attack first: each target packs its own copy of the members and is released before the next
    for s in [int(v) for v in a.grad_steps.split(",") if v]:
        target = EnsembleTarget(cond, states, cfg, mc=a.mc, seed=3, sample_steps=s, eta=1.0)
        ms = median_ms(lambda: target.input_grad(x, labels, check_labels=False), a.warmup, a.repeat)
        r["input_grad"][f"S{s}"] = {"ms": ms, "steps": target.steps}
        print(f"input_grad S={target.steps}: {ms:.1f} ms", flush=True)
        del target
        torch.cuda.empty_cache()

    run = Diffusion(ns(seed=3, mc_trials=a.mc), cfg, device=dev, conditioner=cond, noise_estimator_states=states)
    run.load_noise_estimators(max_batch=a.B, mc_trials=a.mc)
    del states
    noise = torch.randn(a.K, a.T, a.B * a.mc, C, device=dev, generator=torch.Generator(device=dev).manual_seed(5))

    def measure(key, request):
        run.use_sampler(request)
        S = run.sample_steps
        nz = noise[:, :S].contiguous()
        out = run.predict_batch(x, noise=nz)
        entry = {"steps": S, "prob": out["prob"], "vote": out["vote"]}
        entry["ms"] = median_ms(lambda: run.predict_batch(x, noise=nz, clone=False), a.warmup, a.repeat)
        print(f"predict_batch {key}: {S} steps, {entry['ms']:.2f} ms", flush=True)
        return entry

    full = measure("full", None)
    r["predict_batch"]["full"] = {"steps": full["steps"], "ms": full["ms"]}
    for s in [int(v) for v in a.steps.split(",") if v]:
        for eta in (0.0, 1.0):
            key = f"S{s}_eta{int(eta)}"
            e = measure(key, {"steps": s, "skip_type": "uniform", "eta": eta})
            r["predict_batch"][key] = {"steps": e["steps"], "eta": eta, "ms": e["ms"], "speedup": full["ms"] / e["ms"],
                                       "max_prob_diff": float((e["prob"] - full["prob"]).abs().max()),
                                       "equal_votes": float((e["vote"] == full["vote"]).float().mean())}
    r["default_path"] = {"metric": "bench.py --gpus 1 value (denoising-step*images/s), no plan set", "this": bench_values(a.bench_this),
                         "parent": bench_values(a.bench_parent)}
    line = json.dumps(r)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
