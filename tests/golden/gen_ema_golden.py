"""Writes tests/golden/ema.npz: the reference's EMA shadow (diffusion/ema.py, class EMA) walked through a recorded parameter sequence.

Runs only beside a reference checkout (/root/reference, which is not part of the repository and never travels to a GPU box).
diffusion/ema.py is imported UNMODIFIED (it needs torch alone); a small nn.Linear is registered, its parameters are overwritten with
the recorded values before every update(), and the shadow after each update is stored.  Only arrays are written: no reference text.

    rates   [R]        float64   the mu of each walk (0.9999: the shipped configs' ema_rate; 0.5: both products exact, a large step)
    params  [U + 1, n] float32   params[0]: the parameters at register(); params[u]: the parameters at update u = 1 .. U
                                 (named_parameters() order: weight [32, 15] flattened, then bias [32])
    shadow  [R, U, n]  float32   the shadow after update u of walk r

The ordinary values (the weight) change scale from update to update, so that (1 - mu) * w and mu * s are often of one magnitude: there
a contracted multiply-add and an unrounded product differ, and so does 1.0f - (float)mu from (float)(1.0 - mu).  The bias holds the
special values -- +-0, +-inf, NaN, denormals (1e-40, the smallest one, a value whose product with 1e-4 is denormal), FLT_MIN, FLT_MAX --
and moves them one slot every second update, so that the shadow meets each of them from a different neighbour.

Usage:  python tests/golden/gen_ema_golden.py            write tests/golden/ema.npz
        python tests/golden/gen_ema_golden.py --check    regenerate and compare with the COMMITTED file, bit for bit (exit 1 on a difference)
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "ema.npz")
RATES = (0.9999, 0.5)
UPDATES = 8
N_OUT, N_IN = 32, 15                                           # nn.Linear(15, 32): 480 weights + 32 biases
SCALES = (1.0, 3.0e3, 1.0e-3, 7.0e3, 1.0, 2.0e4, 5.0e-2, 9.0e3, 1.0)     # of params[0 .. U]'s ordinary values
FLT_MAX, FLT_MIN = float(np.finfo(np.float32).max), float(np.finfo(np.float32).tiny)
SPECIALS = (0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1e-40, -1e-40, 1.4e-45, 5e-35, -5e-35, FLT_MIN, -FLT_MIN, FLT_MAX,
            -FLT_MAX, 1.0, -1.0, 1e-38, 3e-41, 1e4, -1e-4, 0.0, 1e-40, float("inf"), 1.0, FLT_MAX, 0.0, -0.0, 2e-45, 1e30, -1e30, 0.5,
            float("-inf"))


def reference_ema():
    spec = importlib.util.spec_from_file_location("reference_ema", os.path.join(REF, "diffusion", "ema.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.EMA


def parameter_sequence() -> np.ndarray:
    assert len(SPECIALS) == N_OUT and len(SCALES) == UPDATES + 1
    rng = np.random.RandomState(20240917)
    special = np.array(SPECIALS, dtype=np.float64).astype(np.float32)
    rows = []
    for u in range(UPDATES + 1):
        weight = (rng.standard_normal(N_OUT * N_IN) * SCALES[u]).astype(np.float32)
        rows.append(np.concatenate([weight, np.roll(special, u // 2)]))
    return np.stack(rows)


def generate() -> dict:
    EMA = reference_ema()
    params = parameter_sequence()
    torch.set_flush_denormal(False)
    shadow = np.zeros((len(RATES), UPDATES, params.shape[1]), dtype=np.float32)

    def put(module, row):
        with torch.no_grad():
            module.weight.copy_(torch.from_numpy(row[:N_OUT * N_IN].reshape(N_OUT, N_IN).copy()))
            module.bias.copy_(torch.from_numpy(row[N_OUT * N_IN:].copy()))

    for r, mu in enumerate(RATES):
        module = torch.nn.Linear(N_IN, N_OUT)
        put(module, params[0])
        ema = EMA(mu=mu)
        ema.register(module)
        for u in range(1, UPDATES + 1):
            put(module, params[u])
            ema.update(module)
            sd = ema.state_dict()
            shadow[r, u - 1] = np.concatenate([sd["weight"].numpy().reshape(-1), sd["bias"].numpy().reshape(-1)])
    return {"rates": np.array(RATES, dtype=np.float64), "params": params, "shadow": shadow}


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="regenerate and compare with the committed fixture")
    a = ap.parse_args()
    if not os.path.isdir(REF):
        print(f"{REF} is not here: the fixture can only be made beside a reference checkout", file=sys.stderr)
        return 2
    new = generate()
    if not a.check:
        np.savez_compressed(OUT, **new)
        print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
        return 0
    old = np.load(OUT)
    diffs = [k for k in new if k not in old.files or not same_bits(new[k], old[k])] + [k for k in old.files if k not in new]
    print(f"checked {len(new)} arrays against {OUT}: {'identical' if not diffs else 'different: ' + ', '.join(diffs)}")
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())
