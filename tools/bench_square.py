"""What a Square-attack query costs at ViT-B/16: ms per query of the full loop on the window kernels (nd_square_propose / accept / commit),
of `forward` alone, and of the same loop written as autoattack's whole-array torch ops on the same forward, at s = 200 and s = 6; then
both attack sides alone (scores held fixed, no forward).  Labels are the model's own predictions and eps is tiny, so no row is ever
fooled: every row stays active in both forms for the whole window.  Host clock around a synchronised window; the forms alternate inside
every repetition and the minimum is reported.  One JSON line.

    python tools/bench_square.py [--batch 32] [--queries 30] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nested_diffusion_amd import ops  # noqa: E402
from nested_diffusion_amd.mapping import VisionTransformer  # noqa: E402
from oracle import ref_cpu  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--queries", type=int, default=30, help="queries per timed window")
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_square needs the GPU"
DEV = "cuda"
B, EPS, SEED, N, WARM, REPS = args.batch, 1e-4, 5, args.queries, 5, args.reps
torch.manual_seed(0)
vp = ref_cpu.init_vit_params()                     # ViT-B/16, 224, 2 classes
vit = VisionTransformer(vp, 12, DEV)
x = torch.rand(B, 3, 224, 224, device=DEV)
y = vit.forward(x).argmax(dim=1)
index = torch.arange(B, device=DEV)


def margin_and_loss(logits, y):
    u = torch.arange(logits.shape[0], device=logits.device)
    logits = logits.clone()
    y_corr = logits[u, y].clone()
    logits[u, y] = -float("inf")
    y_others = logits.max(dim=-1)[0]
    return y_corr - y_others, y_corr - y_others


class KernelForm:
    def __init__(self, predict=True):
        self.predict = predict
        self.x_best, self.x_new = ops.square_init(x, index, EPS, SEED)
        self.st = ops.SquareState(B, DEV)
        self.scores = vit.forward(self.x_new)
        ops.square_accept(self.scores, y, self.st, -1)
        self.i = 0

    def query(self, s):
        ops.square_propose(x, self.x_best, self.x_new, index, self.st, s, self.i, EPS, SEED)
        scores = vit.forward(self.x_new) if self.predict else self.scores
        ops.square_accept(scores, y, self.st, self.i)
        ops.square_commit(self.x_best, self.x_new, self.st, s)
        self.i += 1


class TorchForm:
    """autoattack's square.py, Linf branch, as it is written there (one window and one sign per channel for the batch)."""

    def __init__(self, predict=True):
        self.predict = predict
        c, w = 3, 224
        self.x_best = torch.clamp(x + EPS * (2 * torch.randint(0, 2, [B, c, 1, w], device=DEV).float() - 1), 0., 1.)
        self.scores = vit.forward(self.x_best)
        self.margin_min, self.loss_min = margin_and_loss(self.scores, y)
        self.n_queries = torch.ones(B, device=DEV)

    def query(self, s):
        idx_to_fool = (self.margin_min > 0.0).nonzero().flatten()
        x_curr, x_best_curr, y_curr = x[idx_to_fool], self.x_best[idx_to_fool], y[idx_to_fool]
        margin_min_curr, loss_min_curr = self.margin_min[idx_to_fool], self.loss_min[idx_to_fool]
        vh, vw = int(torch.randint(0, 224 - s + 1, [1])), int(torch.randint(0, 224 - s + 1, [1]))
        x_new = x_best_curr.clone()
        x_new[:, :, vh:vh + s, vw:vw + s] = x_curr[:, :, vh:vh + s, vw:vw + s] + EPS * (2 * torch.randint(0, 2, [3, 1, 1], device=DEV).float() - 1)
        x_new = torch.min(torch.max(x_new, x_curr - EPS), x_curr + EPS)
        x_new = torch.clamp(x_new, 0., 1.)
        scores = vit.forward(x_new) if self.predict else self.scores[idx_to_fool]
        margin, loss = margin_and_loss(scores, y_curr)
        idx_improved = (loss < loss_min_curr).float()
        self.loss_min[idx_to_fool] = idx_improved * loss + (1. - idx_improved) * loss_min_curr
        idx_miscl = (margin <= 0.).float()
        idx_improved = torch.max(idx_improved, idx_miscl)
        self.margin_min[idx_to_fool] = idx_improved * margin + (1. - idx_improved) * margin_min_curr
        idx_improved = idx_improved.reshape([-1, 1, 1, 1])
        self.x_best[idx_to_fool] = idx_improved * x_new + (1. - idx_improved) * x_best_curr
        self.n_queries[idx_to_fool] += 1.


class PredictOnly:
    def __init__(self):
        self.x_new = x.clone()

    def query(self, s):
        vit.forward(self.x_new)


def timed(obj, s, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        obj.query(s)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


forms = {"kernel_loop": KernelForm(True), "predict": PredictOnly(), "torch_loop": TorchForm(True),
         "kernel_attack_side": KernelForm(False), "torch_attack_side": TorchForm(False)}
out = {"tool": "bench_square", "batch": B, "model": "vit_base_patch16_224", "queries_per_window": N, "reps": REPS}
for s in (200, 6):
    for f in forms.values():
        timed(f, s, WARM)
    res = {k: [] for k in forms}
    for _ in range(REPS):                                          # alternate the forms inside every repetition
        for k, f in forms.items():
            res[k].append(timed(f, s, N))
    out[f"s={s}"] = {k: {"ms_per_query_min": min(v), "ms_per_query_all": [round(t, 4) for t in v]} for k, v in res.items()}
    print(f"s={s}: " + ", ".join(f"{k} {min(v):.3f} ms" for k, v in res.items()), file=sys.stderr, flush=True)
kf = forms["kernel_loop"]
out["active_rows_at_end"] = {"kernel": int((kf.st.margin_min > 0).sum()), "torch": int((forms["torch_loop"].margin_min > 0).sum())}
print(json.dumps(out))
