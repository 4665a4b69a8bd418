"""Milliseconds per EnsembleTarget.input_grad at the config's own shape, and where they go.

    python tools/bench_ensemble_grad.py [--K 5] [--T 100] [--B 32] [--mc 1] [--warmup 2] [--repeat 7] [--out FILE]

Synthetic weights of the reference's shapes (ViT-B/16, five mapping MLPs, K noise estimators with D = 150528, H = F = 4096), one GPU.
Every figure is the median of `repeat` timed runs after `warmup` untimed ones, each run bracketed by a device synchronisation and timed
on the host: the chain is launched operator by operator from Python, so host time IS part of what a caller waits for.  Prints one JSON
line: input_grad_ms, predict_batch_ms (the same process, the same weights, for scale) and the split -- conditioner chain (recorded
forward + backward), encoders (forward + backward of encoder_x and norm, all members), the K T step forwards, the K T step backwards, and
the loss head."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=5)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--mc", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args(argv)
    from nested_diffusion_amd import ops, synthetic
    from nested_diffusion_amd.mapping import Classifier, GuidingConditioner, VisionTransformer
    from nested_diffusion_amd.runner import Diffusion
    ns = types.SimpleNamespace
    dev, C, D, H, F, img = "cuda", 2, 150528, 4096, 4096, 224
    cfg = ns(data=ns(dataset="ChestXRay", num_classes=C), model=ns(data_dim=D, hidden_dim=H, feature_dim=F, arch="linear"),
             diffusion=ns(timesteps=a.T, beta_schedule="linear", beta_start=1e-4, beta_end=0.02, aux_cls=ns(arch="sevit"),
                          trained_aux_cls_ckpt_path="", trained_diffusion_ckpt_path=[[]], include_guidance=True),
             testing=ns(batch_size=a.B))
    cond = GuidingConditioner(VisionTransformer(synthetic.vit_state(1, device=dev), 12, dev),
                              [Classifier(synthetic.classifier_state(196 * 768, 10 + k, device=dev), dev) for k in range(a.K)])
    states = [synthetic.cond_model_state(D, H, F, C, a.T, 40 + k, device=dev, denoiser=True) for k in range(a.K)]
    run = Diffusion(ns(seed=3, mc_trials=a.mc), cfg, device=dev, conditioner=cond, noise_estimator_states=states)
    target = run.ensemble_target(mc=a.mc)
    run.load_noise_estimators(max_batch=a.B, mc_trials=a.mc)
    del states
    x = synthetic.images(a.B, device=dev)
    labels = torch.arange(a.B, device=dev) % C
    K, M = len(target.tapes), a.B * a.mc
    noise = target.fix_noise(B=a.B)
    x_flat = x.reshape(a.B, D)
    yhat = ops.softmax_rows(torch.randn(K, a.B, C, device=dev))
    dlogits = torch.randn(K, a.B, C, device=dev) * 1e-3
    dy0 = torch.randn(M, C, device=dev) * 1e-3

    def encoders():
        for t in target.tapes:
            w, s, c = t.w, t.a, t.c
            e0 = ops.linear(x_flat, w["enc0"], c["enc0"][0], act="softplus", scale=s["enc0"][0])
            e1 = ops.linear(e0, w["enc3"], c["enc3"][0], act="softplus", scale=s["enc3"][0])
            xe = ops.linear(e1, w["enc6"], c["enc6"][0], scale=s["enc6"][0])
            dn = ops.cond_act_grad(xe, None, s["enc6"][0], a.B)
            du1 = ops.cond_act_grad(ops.linear_grad_input(dn, w["enc6"]), e1, s["enc3"][0], a.B)
            du0 = ops.cond_act_grad(ops.linear_grad_input(du1, w["enc3"]), e0, s["enc0"][0], a.B)
            ops.linear_grad_input(du0, w["enc0"])

    def conditioner():
        logits, tape = cond.forward_recorded(x, target.members)
        cond.backward(tape, dlogits)

    def forwards():
        for i, t in enumerate(target.tapes):
            t.forward(x_flat, yhat[i], noise[i])

    def backwards():                                       # each needs a fresh tape: the forwards are re-run untimed by the caller below
        for t in target.tapes:
            t.backward(dy0)

    r = {"shape": dict(K=K, T=a.T, B=a.B, mc=a.mc, D=D, H=H, F=F), "warmup": a.warmup, "repeat": a.repeat}
    r["input_grad_ms"] = median_ms(lambda: target.input_grad(x, labels, check_labels=False), a.warmup, a.repeat)
    r["predict_batch_ms"] = median_ms(lambda: run.predict_batch(x, mc_trials=a.mc, clone=False), a.warmup, a.repeat)
    r["conditioner_chain_ms"] = median_ms(conditioner, a.warmup, a.repeat)
    r["encoders_ms"] = median_ms(encoders, a.warmup, a.repeat)
    fwd = median_ms(forwards, a.warmup, a.repeat)
    bwd = []
    for i in range(a.warmup + a.repeat):
        forwards()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        backwards()
        torch.cuda.synchronize()
        if i >= a.warmup:
            bwd.append((time.perf_counter() - t0) * 1e3)
    enc_half = r["encoders_ms"] / 2                        # the encoder's forward and backward stream the same three matrices
    r["step_forwards_ms"] = fwd - enc_half
    r["step_backwards_ms"] = statistics.median(bwd) - enc_half
    r["ms_per_step_forward"] = r["step_forwards_ms"] / (K * a.T)
    r["ms_per_step_backward"] = r["step_backwards_ms"] / (K * a.T)
    samples = torch.randn(K * a.mc, a.B, C, device=dev)
    r["loss_head_ms"] = median_ms(lambda: ops.aggregate_xent_grad(samples, target.temperature, labels, check_labels=False), a.warmup, a.repeat)
    # launches per step and member, from the chain's listing: forward 4 nd_linear + nd_cond_mul + nd_reverse_step, backward
    # nd_reverse_step_bwd + 4 nd_linear_bwd + 3 nd_cond_act_bwd
    r["launches_per_step"] = {"forward": 6, "backward": 8}
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
