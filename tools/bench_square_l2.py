"""What the attack side of an L2 Square-attack query costs beside the forward pass it sits around, at the shape of an attacked evaluation:
B = 32, 3 x 224 x 224, ViT-B/16, at the first side of the schedule (s = 201) and the last (s = 9).

    python tools/bench_square_l2.py [--batch 32] [--reps 7] [--big 160] [--out profiles/square_l2_bench.json]

Prints one JSON line (and writes it to --out): us per nd_square_l2_propose (its four launches), per nd_square_accept, per
nd_square_l2_commit with every row accepted (the most it can copy) and per attack side of a query (propose + accept + commit, every row
active and accepted: the label's score falls with every query); ms per ViT-B/16 forward of the same batch; the attack side's share of a
query (attack side + forward) and the rate it achieves against the bytes its passes move: the masked sums read x0 and x_best (2 arrays),
the write reads them again and writes x_new (3), the commit reads x_new and writes x_best (2): 7 arrays of 4 B x B x 150528, plus the two
window passes (2 x 2 windows of 4 B x B x 3 x s x s).  At B = 32 the three arrays are 58 MB and fit the Infinity Cache; --big B repeats
the propose at a batch whose arrays do not (160: 289 MB), for the per-image cost with and without it.  Warm-up first, medians over --reps
windows of 50 calls, host clock around a synchronised window.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CALLS = 50


def timed(fn, reps):
    """ms per call: `reps` windows of CALLS calls"""
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(CALLS):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3 / CALLS)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--big", type=int, default=160, help="a second batch size whose arrays exceed the Infinity Cache (0: skip)")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "square_l2_bench.json"))
    a = ap.parse_args()
    from nested_diffusion_amd import ops
    from nested_diffusion_amd.mapping import VisionTransformer
    from nested_diffusion_amd.square import SquareL2Attack
    from oracle import ref_cpu
    assert torch.cuda.is_available(), "bench_square_l2 needs the GPU"
    dev, eps, seed, Cin, H, W = "cuda", 2.0, 5, 3, 224, 224
    med = statistics.median
    vit = VisionTransformer(ref_cpu.init_vit_params(embed=768, depth=12, img=224, seed=1), 12, dev)
    atk = SquareL2Attack(vit, eps=eps, seed=seed)
    r = {"tool": "bench_square_l2", "batch": a.batch, "model": "vit_base_patch16_224", "reps": a.reps, "calls_per_window": CALLS,
         "device": torch.cuda.get_device_name(0)}

    def setup(B):
        x = torch.rand(B, Cin, H, W, generator=torch.Generator().manual_seed(2)).to(dev)
        index = torch.arange(B, device=dev)
        x_best, x_new, _ = ops.square_l2_init(x, index, atk.eta(min(H, W) // 5, dev), eps, seed)
        st = ops.SquareL2State(B, Cin, H, W, dev)
        y = torch.zeros(B, dtype=torch.int64, device=dev)
        first = torch.tensor([[1e6, 0.0]], device=dev).repeat(B, 1).contiguous()
        ops.square_accept(first, y, st, -1)                        # margin 1e6: every row active
        return x, index, x_best, x_new, st, y

    B = a.batch
    x, index, x_best, x_new, st, y = setup(B)
    # scores whose margin falls with every call (and stays positive): every query is an improvement, every row is accepted
    falling = [torch.tensor([[1e5 - k, 0.0]], device=dev).repeat(B, 1).contiguous() for k in range(CALLS * (a.reps + 2) * 2 + 8)]
    forward = lambda: vit.forward(x_new)                                                                                      # noqa: E731
    for _ in range(3):
        forward()
    CALLS_FWD, t_fwd = 5, []                                       # a forward is milliseconds: five per window are enough
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(CALLS_FWD):
            forward()
        torch.cuda.synchronize()
        t_fwd.append((time.perf_counter() - t) * 1e3 / CALLS_FWD)
    r["forward_ms"] = med(t_fwd)
    per_array = 4.0 * B * Cin * H * W
    k = [0]
    for s in (201, 9):
        eta = atk.eta(s, dev)
        propose = lambda: ops.square_l2_propose(x, x_best, x_new, index, st, eta, s, 3, eps, seed)                            # noqa: E731
        commit = lambda: ops.square_l2_commit(x_best, x_new, st)                                                             # noqa: E731

        def accept():
            ops.square_accept(falling[k[0]], y, st, 3)
            k[0] += 1

        def side():
            propose()
            accept()
            commit()

        side()
        assert int((st.flags == ops.SQUARE_ACTIVE | ops.SQUARE_ACCEPT).sum()) == B                # every row accepted: the commit copies all
        t_side = timed(side, a.reps)
        assert int((st.flags == ops.SQUARE_ACTIVE | ops.SQUARE_ACCEPT).sum()) == B
        t_prop, t_commit = timed(propose, a.reps), timed(commit, a.reps)
        k[0] = 0
        ops.square_accept(torch.tensor([[1e6, 0.0]], device=dev).repeat(B, 1).contiguous(), y, st, -1)
        t_acc = timed(accept, 2)
        k[0] = 0
        ops.square_accept(torch.tensor([[1e6, 0.0]], device=dev).repeat(B, 1).contiguous(), y, st, -1)
        bytes_side = 7 * per_array + 2 * 2 * 4.0 * B * Cin * s * s
        side_ms = med(t_side)
        r[f"s{s}"] = {"attack_side_us": side_ms * 1e3, "propose_us": med(t_prop) * 1e3, "accept_us": med(t_acc) * 1e3,
                      "commit_us": med(t_commit) * 1e3, "attack_side_share_percent": 100.0 * side_ms / (side_ms + r["forward_ms"]),
                      "bytes_attack_side": bytes_side, "attack_side_gbps": bytes_side / side_ms / 1e6,
                      "propose_gbps": (5 * per_array + 2 * 2 * 4.0 * B * Cin * s * s) / med(t_prop) / 1e6,
                      "commit_gbps": 2 * per_array / med(t_commit) / 1e6,
                      "propose_us_per_image": med(t_prop) * 1e3 / B}
    if a.big:
        del falling
        Bb = a.big
        xb, indexb, x_bestb, x_newb, stb, _ = setup(Bb)
        for s in (201, 9):
            eta = atk.eta(s, dev)
            propose = lambda: ops.square_l2_propose(xb, x_bestb, x_newb, indexb, stb, eta, s, 3, eps, seed)                   # noqa: E731
            propose()
            t = med(timed(propose, a.reps))
            r[f"s{s}"]["big_batch"] = Bb
            r[f"s{s}"]["big_propose_us"] = t * 1e3
            r[f"s{s}"]["big_propose_us_per_image"] = t * 1e3 / Bb
            r[f"s{s}"]["big_propose_gbps"] = (5 * 4.0 * Bb * Cin * H * W + 2 * 2 * 4.0 * Bb * Cin * s * s) / t / 1e6
    line = json.dumps(r)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
