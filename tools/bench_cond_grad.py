"""The conditioner input gradient at config dims (ViT-B/16 prefix, five 150528 -> 4096 -> 2048 -> 128 -> 2 mapping MLPs, B = 32): one
GuidingConditioner.input_grad and its parts, and the new weight stream against its yardstick -- the forward nd_linear of the same
layer, timed in the same process in alternating windows (both stream the same 2.47 GB image once).  GPU only.

    python tools/bench_cond_grad.py [--batch 32] [--reps 200] [--rounds 5] [--linear-only] [--out FILE]

Prints one JSON line (and writes it to --out): times in ms (median over the rounds, each a window of `reps` calls between two device
events), bwd_over_fwd, and the TB/s of each stream = image bytes / time."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nested_diffusion_amd import ops, synthetic  # noqa: E402
from nested_diffusion_amd.mapping import Classifier, GuidingConditioner, VisionTransformer  # noqa: E402


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
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--linear-only", action="store_true", help="the weight stream and its yardstick only (one member's layer 1)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_cond_grad needs the GPU: there is nothing to measure without one")
    dev, B, E, N_TOK, K_MEM = "cuda", a.batch, 768, 196, 5
    mlps = [Classifier(synthetic.classifier_state(N_TOK * E, seed=2000 + k, device=dev), dev) for k in range(1 if a.linear_only else K_MEM)]

    # the stream and its yardstick: layer 1 of member 0, M = B
    w1, b1 = mlps[0].p["linear1.weight"], mlps[0].p["linear1.bias"]
    x1 = torch.randn(B, w1.K, device=dev)
    dy1 = torch.randn(B, w1.N, device=dev)
    add1 = torch.randn(B, w1.K, device=dev)
    (t_fwd, t_bwd), (s_fwd, s_bwd) = timed([lambda: ops.linear(x1, w1, b1, act="relu"),
                                            lambda: ops.linear_grad_input(dy1, w1, add=add1)], a.reps, a.rounds)
    image_bytes = w1.data.numel() * 4
    res = {"tool": "bench_cond_grad", "batch": B, "members": K_MEM, "layer1": [w1.K, w1.N], "image_gb": round(image_bytes / 1e9, 3),
           "linear_fwd_ms": round(t_fwd, 4), "linear_bwd_ms": round(t_bwd, 4), "bwd_over_fwd": round(t_bwd / t_fwd, 3),
           "linear_fwd_tbps": round(image_bytes / t_fwd / 1e9, 3), "linear_bwd_tbps": round(image_bytes / t_bwd / 1e9, 3),
           "linear_fwd_ms_min_max": [round(v, 4) for v in s_fwd], "linear_bwd_ms_min_max": [round(v, 4) for v in s_bwd],
           "reps": a.reps, "rounds": a.rounds}
    if not a.linear_only:
        res.update(parts(a, dev, B, E, N_TOK, K_MEM, mlps, w1))
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


def parts(a, dev, B, E, N_TOK, K_MEM, mlps, w1):
    """one input_grad and its parts, ms"""
    vit = VisionTransformer(synthetic.vit_state(seed=7, device=dev), 12, dev)
    cond = GuidingConditioner(vit, mlps)
    img = synthetic.images(B, device=dev)
    labels = torch.arange(B, device=dev) % 2
    vit.transposed_weights()
    add1 = torch.randn(B, w1.K, device=dev)
    # the parts of one input_grad
    state = {}

    def prefix_fwd():
        tok, recs, toks = vit.patch_embed(img), [], []
        for i in range(K_MEM):
            recs.append({})
            tok = vit.block(i, tok, B, rec=recs[-1])
            toks.append(tok)
        state.update(recs=recs, toks=toks)

    def mlp_fwd():
        state["heads"] = [mlps[i].forward_recorded(state["toks"][i]) for i in range(K_MEM)]

    d1 = [torch.randn(B, w1.N, device=dev) for _ in range(K_MEM)]

    def layer1_bwd():
        for i in range(K_MEM):
            ops.linear_grad_input(d1[i], mlps[i].p["linear1.weight"], add=add1)

    dtok0 = torch.randn(B * N_TOK, E, device=dev)

    def prefix_bwd():
        dtok, dimg = dtok0, ops.split_rows(dtok0)
        for i in range(K_MEM - 1, -1, -1):
            dtok, dimg = vit._block_grad(i, state["recs"][i], dtok, dimg, B)
        ops.unpatchify(ops.gemm_split(dimg, vit._wT["patch_embed"]), B, vit.in_chans, 224, 224, vit.patch)

    prefix_fwd()
    mlp_fwd()
    ms, _ = timed([prefix_fwd, mlp_fwd, layer1_bwd, prefix_bwd, lambda: cond.input_grad(img, labels, check_labels=False),
                      lambda: cond.compute_guiding_prediction(img, include_full_vit=False)], max(a.reps // 10, 3), a.rounds)
    return {"prefix_fwd_ms": round(ms[0], 3), "mlp_fwd_ms": round(ms[1], 3), "layer1_bwd_x5_ms": round(ms[2], 3),
            "prefix_bwd_ms": round(ms[3], 3), "input_grad_ms": round(ms[4], 3), "guiding_prediction_ms": round(ms[5], 3)}


if __name__ == "__main__":
    sys.exit(main())
