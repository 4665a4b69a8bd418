"""Writes the attacked test sets the reference evaluates (its ChestXRayAtk* / ISICSkinCancerAtk* datasets), on the GPU:

    python -m nested_diffusion_amd.make_attacks --config <yml> --attack_name FGSM|PGD|BIM|L2PGD|AUTOPGD|APGDL2|SQUARE|SQUAREL2 --eps E --out ROOT \
        [--preprocess grayscaled] [--seed S] [--batch_size B] [--target vit|conditioner|ensemble] [--members 0,1,...] [--mc N] \
        [--sample_steps N [--skip_type uniform|quadratic] [--eta E]] [--eot N] [--n_queries N]

Loads the ViT checkpoint the runner would load (<trained_aux_cls_ckpt_path>/vit_base_patch16_224_<Dataset>.pth), attacks the config's
test split (the PGD / APGD random start of an image is keyed on its index in the dataset) and writes ROOT/Test_attacks_<NAME>/<class>/<stem>.png
as RGB uint8 = round(255 * adv), with the classes and file stems of the source: the tree data_loader_attacks reads
(dataset_helper/chest_x_ray_dataset.py:197-227; here data.get_dataset with a *Atk<NAME> dataset name).  AUTOPGD is the reference's
AutoAttack(vit, eps=eps, version='custom', norm='Linf', attacks_to_run=['apgd-ce']) run by run_standard_evaluation on each batch.
A Carlini & Wagner set is written from Python: write_attacked_set(config, attack.CarliniWagner(eps, vit, ...), "CW", out); so is a
Square set: write_attacked_set(config, square.SquareAttack(vit, eps=eps), "SQUARE", out) (no dataset name reads that tree back).
--target conditioner attacks the mapping networks the ensemble is conditioned on instead of the full ViT's head (a white-box attack on the
defence's front end): the checkpoints are read by mapping.load_conditioner and wrapped in a mapping.ConditionerTarget, whose loss is the
cross-entropy of the members' averaged softmax; --members selects the members (default: all).
--target ensemble attacks the ensemble itself, end to end (the adaptive white-box attack): the conditioner and the config's noise-estimator
checkpoints (diffusion.trained_diffusion_ckpt_path) are wrapped in an ensemble_grad.EnsembleTarget, whose loss is -log of the probability
test_atk reports, differentiated through the aggregation, the reverse diffusions (--mc trials per member, default 1; batch_size * mc <= 128)
and both paths from the pixels; every gradient step draws fresh sampler noise.  --sample_steps N [--skip_type uniform|quadratic] [--eta E]
attacks the ensemble as `main --test --sample_steps N` runs it: N of the schedule's timesteps per chain (a sampler plan,
diffusion_utils.sampler_plan), in time and in tape.
APGDL2 is autoattack's APGD-CE in the L2 threat model: autoattack.APGDAttack(target, norm='L2', eps, n_restarts=5, n_iter=100, seed); its tree is
Test_attacks_APGDL2 (no dataset name reads it back, as for SQUARE).  --eot N wraps the chosen target in an eot.EOTTarget for any attack name:
every gradient of the attack becomes the mean of N gradients at the same point (the accepted way to attack a randomized defence).  An
EOT-N APGD run on --target ensemble is N x n_iter x n_restarts ensemble gradients: use --sample_steps to keep that affordable.
SQUARE and SQUAREL2 are the score-based attacks square.SquareAttack (Linf) and square.SquareL2Attack (L2) on the chosen target, the control for
gradient masking; --n_queries N (default 5000) is their query budget and is refused with any other attack name.  Their trees are
Test_attacks_SQUARE and Test_attacks_SQUAREL2 (no dataset name reads them back).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="write an attacked test set (Test_attacks_<NAME>) with the GPU attacks of attack.py")
    p.add_argument("--config", type=str, required=True)
    p.add_argument("--attack_name", type=str, choices=["FGSM", "PGD", "BIM", "L2PGD", "AUTOPGD", "APGDL2", "SQUARE", "SQUAREL2"], required=True)
    p.add_argument("--eps", type=float, required=True)
    p.add_argument("--out", type=str, required=True, help="root the Test_attacks_<NAME> tree is written under")
    p.add_argument("--preprocess", type=str, choices=["grayscaled", "standardized"], default="grayscaled")
    p.add_argument("--seed", type=int, default=0, help="key of the PGD / APGD random start")
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--dataroot", type=str, default=None)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--target", type=str, choices=["vit", "conditioner", "ensemble"], default="vit",
                   help="vit: the full ViT's head, as the reference attacks; conditioner: the mapping networks the ensemble is conditioned on; "
                        "ensemble: the whole ensemble, through the sampler")
    p.add_argument("--members", type=str, default=None, help="--target conditioner / ensemble: comma-separated member indices (default: all)")
    p.add_argument("--mc", type=int, default=argparse.SUPPRESS, help="--target ensemble: Monte-Carlo trials per member (default 1)")
    p.add_argument("--sample_steps", type=int, default=argparse.SUPPRESS,
                   help="--target ensemble: reverse steps per chain (a sampler plan over the schedule; default: every timestep)")
    p.add_argument("--skip_type", type=str, default=argparse.SUPPRESS, help="with --sample_steps: uniform (default) or quadratic")
    p.add_argument("--eta", type=float, default=argparse.SUPPRESS, help="with --sample_steps: 0 (deterministic) .. 1 (default, ancestral)")
    p.add_argument("--eot", type=int, default=argparse.SUPPRESS,
                   help="expectation over transformation: every gradient is the mean of N gradients of the target at the same point")
    p.add_argument("--n_queries", type=int, default=argparse.SUPPRESS, help="SQUARE / SQUAREL2: the query budget (default 5000)")
    return p


SQUARE_NAMES = ("SQUARE", "SQUAREL2")


def check_n_queries(args) -> None:
    """--n_queries belongs to the Square attacks: refused by name (SystemExit) with any other attack, and below 1."""
    if not hasattr(args, "n_queries"):
        return
    if args.attack_name not in SQUARE_NAMES:
        raise SystemExit(f"--n_queries is the query budget of --attack_name SQUARE or SQUAREL2 (got {args.attack_name})")
    if args.n_queries < 1:
        raise SystemExit(f"--n_queries must be at least 1 (got {args.n_queries})")


def eot_wrap(args, target):
    """The target itself without --eot, else an eot.EOTTarget of it."""
    if not hasattr(args, "eot"):
        return target
    from .eot import EOTTarget

    return EOTTarget(target, args.eot)


def make_named_attack(args, target):
    """The attack --attack_name names, on `target`."""
    from .attack import make_attack
    from .autoattack import APGDAttack, AutoAttack

    if args.attack_name == "AUTOPGD":
        return AutoAttack(target, eps=args.eps, seed=args.seed, version="custom", norm="Linf", attacks_to_run=["apgd-ce"])
    if args.attack_name == "APGDL2":
        return APGDAttack(target, norm="L2", eps=args.eps, n_restarts=5, n_iter=100, seed=args.seed)
    if args.attack_name in SQUARE_NAMES:
        from .square import SquareAttack, SquareL2Attack

        cls = SquareAttack if args.attack_name == "SQUARE" else SquareL2Attack
        return cls(target, eps=args.eps, n_queries=getattr(args, "n_queries", 5000), seed=args.seed)
    return make_attack(args.eps, args.attack_name, target, seed=args.seed)


def sampler_args(args) -> dict:
    """--sample_steps / --skip_type / --eta as EnsembleTarget's keywords; every misuse is refused by name (SystemExit) before the GPU is touched."""
    from .diffusion_utils import SKIP_TYPES

    if not hasattr(args, "sample_steps"):
        for flag in ("skip_type", "eta"):
            if hasattr(args, flag):
                raise SystemExit(f"--{flag} is read with --sample_steps only")
        return {}
    if args.target != "ensemble":
        raise SystemExit("--sample_steps sets the sampler plan of --target ensemble")
    kw = {"sample_steps": args.sample_steps, "skip_type": getattr(args, "skip_type", "uniform"), "eta": getattr(args, "eta", 1.0)}
    if kw["sample_steps"] < 1:
        raise SystemExit(f"--sample_steps must be at least 1 (got {kw['sample_steps']})")
    if kw["skip_type"] not in SKIP_TYPES:
        raise SystemExit(f"--skip_type must be one of {SKIP_TYPES} (got {kw['skip_type']!r})")
    if not 0.0 <= kw["eta"] <= 1.0:
        raise SystemExit(f"--eta must lie in [0, 1] (got {kw['eta']})")
    return kw


def parse_members(text):
    """'0,2' -> [0, 2]; None -> None (all members)"""
    return None if text is None else [int(t) for t in text.split(",") if t.strip()]


def checkpoint_name(config) -> str:
    """The dataset part of the checkpoint file names the runner would load for the config's dataset."""
    from .runner import CHEST

    base = config.data.dataset.split("Atk", 1)[0].replace("Validate", "")
    return "ChestXRay" if base in CHEST else "ISICSkinCancer"


def load_vit(config, device):
    """The ViT checkpoint the runner would load for the config's dataset."""
    from .mapping import VisionTransformer, load_pickled

    sd = load_pickled(os.path.join(config.diffusion.trained_aux_cls_ckpt_path, f"vit_base_patch16_224_{checkpoint_name(config)}.pth"))
    return VisionTransformer(sd, max(1, sd["patch_embed.proj.weight"].shape[0] // 64), device)


def load_target(config, device, members=None):
    """--target conditioner: the conditioner the runner would load for the config's dataset, as the model of a gradient attack."""
    from .mapping import ConditionerTarget, load_conditioner

    return ConditionerTarget(load_conditioner(config.diffusion.trained_aux_cls_ckpt_path, checkpoint_name(config), device), members)


def load_ensemble_target(config, device, members=None, mc: int = 1, seed: int = 0, **sampler):
    """--target ensemble: the conditioner and the noise estimators the runner would load for the config's dataset, as the model of a gradient
    attack on the whole ensemble (ensemble_grad.EnsembleTarget)."""
    from .ensemble_grad import EnsembleTarget
    from .mapping import load_checkpoint_object, load_conditioner

    cond = load_conditioner(config.diffusion.trained_aux_cls_ckpt_path, checkpoint_name(config), device)
    paths = config.diffusion.trained_diffusion_ckpt_path[0]
    states = [load_checkpoint_object(p)["noise_estimator"] for p in paths[:len(cond.mlps)]]
    return EnsembleTarget(cond, states, config, mc=mc, members=members, seed=seed, **sampler)


def write_attacked_set(config, attack, name: str, out: str, preprocess: str = "grayscaled", batch_size: int = 32, dataroot: str = None,
                       device=None) -> int:
    """Attacks the clean test split of the config's dataset with `attack` (an Attack, an L2Attack, a CarliniWagner, a SquareAttack or SquareL2Attack, an APGDAttack, a
    WorstCase or an AutoAttack, which holds the ViT it attacks) and writes out/Test_attacks_<name>; returns the number of successful attacks."""
    import types

    from PIL import Image

    from .autoattack import AutoAttack
    from .data import get_dataset

    if dataroot is not None:
        config.data.dataroot = dataroot
    config.data.dataset = config.data.dataset.split("Atk", 1)[0].replace("Validate", "")     # the clean test split of the config's dataset
    ds = get_dataset(types.SimpleNamespace(preprocess=preprocess), config)
    vit = attack.model
    device = vit.device if device is None else device
    out_root = os.path.join(out, f"Test_attacks_{name}")
    n_ok = 0
    for start in range(0, len(ds), batch_size):
        idx = list(range(start, min(start + batch_size, len(ds))))
        items = [ds[i] for i in idx]
        x = torch.stack([it[0] for it in items]).to(device)
        y = torch.tensor([it[1] for it in items], dtype=torch.int64, device=device)
        if isinstance(attack, AutoAttack):
            adv = attack.run_standard_evaluation(x, y, bs=len(idx), first_image=start)
            success = vit.forward(adv).argmax(dim=1) != y
        else:
            adv, success = attack.generate_attack(x, y, first_image=start)
        n_ok += int(success.sum())
        pix = torch.round(adv.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().cpu().numpy()
        for k, i in enumerate(idx):
            path, target = ds.samples[i]
            d = os.path.join(out_root, ds.classes[target])
            os.makedirs(d, exist_ok=True)
            stem = os.path.splitext(os.path.basename(path))[0]
            Image.fromarray(np.ascontiguousarray(pix[k]), "RGB").save(os.path.join(d, stem + ".png"))
    print(f"{name} eps={attack.epsilon}: {len(ds)} images written under {out_root}, {n_ok} successful attacks")
    return n_ok


def main(argv=None) -> int:
    from . import main as nd_main

    args = build_parser().parse_args(argv)
    if args.target == "vit" and args.members is not None:
        raise SystemExit("--members selects members of --target conditioner or ensemble")
    if args.target != "ensemble" and hasattr(args, "mc"):
        raise SystemExit("--mc sets the trials of --target ensemble")
    if hasattr(args, "eot") and args.eot < 1:
        raise SystemExit(f"--eot must be at least 1 (got {args.eot})")
    check_n_queries(args)
    sampler = sampler_args(args)
    with open(args.config) as f:
        import yaml
        config = nd_main.dict2namespace(yaml.safe_load(f))
    device = torch.device("cuda", args.device)
    if args.target == "ensemble":
        vit = load_ensemble_target(config, device, parse_members(args.members), getattr(args, "mc", 1), args.seed, **sampler)
    else:
        vit = load_vit(config, device) if args.target == "vit" else load_target(config, device, parse_members(args.members))
    attack = make_named_attack(args, eot_wrap(args, vit))
    write_attacked_set(config, attack, args.attack_name, args.out, args.preprocess, args.batch_size, args.dataroot, device)
    return 0


if __name__ == "__main__":
    sys.exit(main())
