"""Drop-in for the reference's diffusion/main.py on the inference path:

    python -m nested_diffusion_amd.main --test --config configs/chest_x_ray.yml --loss card_onehot_conditional \
        --doc chest_x_ray --preprocess grayscaled --ni [--device N] [--timesteps T] [--seed S] [--exp DIR] ...

Same flags, YAML keys and checkpoint layout as the reference (main.py:16-161, 166-296, 299-380;
canonical invocation testing_scripts/test.sh:24).  Implemented, with loss card_onehot_conditional and
aux_cls.arch == 'sevit' (the shipped configs): `--test`, `--calib`, and -- with neither -- training of the noise
estimator `--mlp_idx` on one GPU (runner.Diffusion.train; `--snapshot_epochs N` keeps the whole training state in
<log_path>/ckpt.pth and `--resume_training` continues from it); the other training / sampling flags are
parsed for compatibility and rejected at dispatch.  Additions: --synthetic_batches, --mc_trials, --snapshot_epochs, --sample_steps, --ema, --use_ema.
`--ema` (training) keeps the reference's EMA shadow of the parameters at model.ema_rate; `--use_ema` (--test, --calib) samples from it.
`--sample_steps N` samples with N of the schedule's timesteps per chain (a sampler plan, diffusion_utils.sampler_plan; not a reference
mode); only then are the reference's declared-and-never-read `--skip_type`, `--sample_type` and `--eta` read (runner.sampler_request).
`--timesteps` is still the reference's override of diffusion.timesteps, which changes the embedding tables' shape.
Multi-GPU: launch with `python -m torch.distributed.run --nproc-per-node N -m nested_diffusion_amd.main ...`.
"""
from __future__ import annotations

import argparse
import logging
import os
import random
import shutil
import sys
import time
import traceback

import numpy as np
import yaml


def build_parser() -> argparse.ArgumentParser:
    """The reference's argparse surface (main.py:16-159), argument for argument."""
    p = argparse.ArgumentParser(description="nested-diffusion inference on MI355X (reference-compatible CLI)")
    p.add_argument('--low_mem_mode', type=bool, required=False, default=False)      # quirk Q9: any non-empty string is True
    p.add_argument('--calib', action="store_true")
    p.add_argument('--fp16', action="store_true",
                   help="(not a reference flag) hold the large weight matrices and their input activations in fp16")
    p.add_argument('--mlp_idx', type=int, required=False)
    p.add_argument('--seed', type=int, required=False)
    p.add_argument('--preprocess', type=str, choices=['grayscaled', 'standardized'], required=True)
    p.add_argument('--noise_perturbation', type=float, required=False, default=0.0)
    p.add_argument('--low_resolution', type=int, required=False, default=0)
    p.add_argument('--brightness', type=float, required=False, default=0.0)
    p.add_argument('--contrast', type=float, required=False, default=1.0)
    p.add_argument('--crop', type=float, required=False, default=0.0)
    p.add_argument('--covered', type=float, nargs=2, required=False, default=(0.0, 0.0))
    p.add_argument('--attack_name', type=str, choices=['None', 'FGSM', 'PGD', 'AUTOPGD'], required=False, default=None)
    p.add_argument('--eps', type=float, required=False)
    p.add_argument("--config", type=str, required=True)
    p.add_argument('--device', type=int, default=0)
    p.add_argument('--thread', type=int, default=4)
    p.add_argument("--test_sample_seed", type=int, default=-1)
    p.add_argument("--exp", type=str, default="exp")
    p.add_argument("--doc", type=str, required=True)
    p.add_argument("--dataroot", type=str, default=None)
    p.add_argument("--comment", type=str, default="")
    p.add_argument("--verbose", type=str, default="info")
    p.add_argument("--test", action="store_true")
    p.add_argument("--tune_T", action="store_true")
    p.add_argument("--sanity_check", action="store_true")
    p.add_argument("--sample", action="store_true")
    p.add_argument("--train_guidance_only", action="store_true")
    p.add_argument("--noise_prior", action="store_true")
    p.add_argument("--no_cat_f_phi", action="store_true")
    p.add_argument("--add_ce_loss", action="store_true")
    p.add_argument("--eval_best", action="store_true")
    p.add_argument("--fid", action="store_true")
    p.add_argument("--interpolation", action="store_true")
    p.add_argument("--resume_training", action="store_true")
    p.add_argument("-i", "--image_folder", type=str, default="images")
    p.add_argument("--n_splits", type=int, default=10)
    p.add_argument("--split", type=int, default=0)
    p.add_argument("--ni", action="store_true")
    p.add_argument("--sample_type", type=str, default="generalized")
    p.add_argument("--skip_type", type=str, default="uniform")
    p.add_argument("--timesteps", type=int, default=None)
    p.add_argument("--eta", type=float, default=0.0)
    p.add_argument("--sequence", action="store_true")
    p.add_argument("--loss", type=str, default='ddpm')
    p.add_argument("--num_sample", type=int, default=1)
    # additions of this build (no reference counterpart)
    p.add_argument("--synthetic_batches", type=int, default=0, help="run on N synthetic test batches instead of a disk dataset")
    p.add_argument("--mc_trials", type=int, default=20, help="Monte-Carlo trials per member (hard-coded 20 in the reference)")
    p.add_argument("--sample_steps", type=int, default=argparse.SUPPRESS,
                   help="sample with N of the schedule's timesteps per chain (--test, --calib); then --skip_type uniform|quadratic, "
                        "--sample_type generalized|ddpm_noisy (eta = 1) and --eta in [0, 1] are read.  Not given: every timestep, as always "
                        "(and no attribute is left behind)")
    p.add_argument("--train_cache", type=str, default="none", choices=["none", "device"],
                   help="training (--mlp_idx k): 'device' decodes every image once, keeps both splits on the GPU as bytes and gathers each "
                        "batch there (same batches, same weights); 'none' decodes every epoch in a DataLoader")
    p.add_argument("--cache_dir", type=str, default=None, help="with --train_cache device: keep the decoded sets here and reuse them in later runs")
    p.add_argument("--snapshot_epochs", type=int, default=argparse.SUPPRESS,
                   help="training (--mlp_idx k): write the whole training state (weights, Adam's moments, counters, generators) to "
                        "<log_path>/ckpt.pth every N epochs and after the last one; --resume_training continues from that file "
                        "(default 0: never; a flag that is not given leaves no attribute behind)")
    p.add_argument("--ema", action="store_true", default=argparse.SUPPRESS,
                   help="training (--mlp_idx k): keep the reference's EMA shadow of the parameters at the config's model.ema_rate, updated in "
                        "the optimizer's pass; the best checkpoint gains an 'ema' entry and ckpt.pth carries the shadow.  Not given: no shadow, "
                        "whatever model.ema says in the config (and no attribute is left behind)")
    p.add_argument("--use_ema", action="store_true", default=argparse.SUPPRESS,
                   help="--test / --calib: read the 'ema' entry of the noise-estimator checkpoints (written by --ema) instead of "
                        "'noise_estimator' (not given: the live weights, and no attribute is left behind)")
    return p


def dict2namespace(config):
    """main.py:288-296."""
    namespace = argparse.Namespace()
    for key, value in config.items():
        setattr(namespace, key, dict2namespace(value) if isinstance(value, dict) else value)
    return namespace


def load_config(args):
    """main.py:169-194: YAML -> nested Namespace plus the CLI overrides (--dataroot, --noise_prior, --no_cat_f_phi,
    --timesteps, --num_sample).  Host-only: touches neither the file system beyond the YAML nor the GPU."""
    with open(args.config, "r") as f:
        if args.sample:
            raise NotImplementedError("--sample: NotImplementedError in the reference as well (main.py:246)")
        new_config = dict2namespace(yaml.safe_load(f))
    if args.dataroot is not None:
        new_config.data.dataroot = args.dataroot
    new_config.diffusion.noise_prior = True if args.noise_prior else False
    new_config.model.cat_y_pred = False if args.no_cat_f_phi else True
    if not args.resume_training:
        if args.timesteps is not None:
            new_config.diffusion.timesteps = args.timesteps            # main.py:192-193
        if args.num_sample > 1:
            new_config.diffusion.num_sample = args.num_sample
    return new_config


def parse_config(args):
    """main.py:166-285 for the --test path: YAML -> Namespace, CLI overrides, log dirs, logger, seeds, device."""
    import torch
    args.log_path = os.path.join(args.exp, "logs", args.doc)
    new_config = load_config(args)
    rank = int(os.environ.get("RANK", "0"))
    if not args.resume_training:
        if rank == 0:
            if os.path.exists(args.log_path):
                if not args.ni:
                    response = input("Folder already exists. Overwrite? (Y/N)")
                    if response.upper() != "Y":
                        print("Folder exists. Program halted.")
                        sys.exit(0)
                shutil.rmtree(args.log_path)
            os.makedirs(args.log_path)
            with open(os.path.join(args.log_path, "config.yml"), "w") as f:
                yaml.dump(new_config, f, default_flow_style=False)
    new_config.tb_logger = None
    level = getattr(logging, args.verbose.upper(), None)
    if not isinstance(level, int):
        raise ValueError("level {} not supported".format(args.verbose))
    formatter = logging.Formatter("%(levelname)s - %(filename)s - %(asctime)s - %(message)s")
    logger = logging.getLogger()
    h1 = logging.StreamHandler()
    h1.setFormatter(formatter)
    logger.addHandler(h1)
    if rank == 0 and os.path.isdir(args.log_path):
        h2 = logging.FileHandler(os.path.join(args.log_path, "stdout.txt"))
        h2.setFormatter(formatter)
        logger.addHandler(h2)
    logger.setLevel(level)
    local = int(os.environ.get("LOCAL_RANK", str(args.device)))
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: the HIP path has no CPU fallback (the reference falls back to cpu at main.py:272)")
    device = torch.device(f"cuda:{local}")
    logging.info("Using device: {}".format(device))
    new_config.device = device
    set_seed(args.seed)
    return new_config, logger


def set_seed(seed: int) -> None:
    """main.py:277-281 (torch, numpy, cuda); the runner's own set_seed (classification_train_separately.py:31-38, from
    Diffusion.__init__) adds python `random`, which random_cover_new's rectangles come from.  All ranks of a multi-GPU
    run use the same seed: the runner makes the random draws of a WHOLE batch and applies its own rows of them (runner.perturb / draw_noise)."""
    from .runner import set_seed as runner_set_seed
    runner_set_seed(seed)


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    from .runner import sampler_request
    try:
        sampler_request(args)                                     # every misuse of --sample_steps and its three flags, before the GPU is touched
    except ValueError as e:
        raise SystemExit(str(e))
    if args.seed is None:
        args.seed = random.randint(0, 10000)                      # main.py:163-164
    args.doc = args.doc + "/split_" + str(args.split)             # main.py:384
    # --thread (main.py:40; parsed by the reference and never used, quirk Q10; test.sh passes 8): the host-side torch work here is
    # decode, staging copies and tiny tensors -- on a box that shows hundreds of logical CPUs under a container quota torch's default
    # (all of them) makes a 19 MB copy take 20-60 ms instead of 2, so the flag bounds the intra-op threads of this process
    if getattr(args, "thread", 0) and args.thread > 0:
        import torch
        torch.set_num_threads(int(args.thread))
    from . import dist as nd_dist
    _, _, world = nd_dist.init_from_env()
    failed = False
    try:
        config, logger = parse_config(args)
    except BaseException:
        nd_dist.shutdown()
        raise
    logging.info("Writing log file to {}".format(args.log_path))
    logging.info("Exp instance id = {}".format(os.getpid()))
    if args.loss != 'card_onehot_conditional':
        # main.py:305-311: raised BEFORE the reference's try block, so the process dies with a traceback and a non-zero exit code
        nd_dist.shutdown()
        raise NotImplementedError("Invalid loss option")
    try:
        from .runner import Diffusion
        runner = Diffusion(args, config, device=config.device)
        start_time = time.time()
        if args.test:
            runner.test_atk()
            procedure = "Testing"
        elif args.calib:
            from scipy.optimize import minimize                      # main.py:356-361
            res = minimize(runner.test_calibrate, 0.2555, method='Nelder-Mead', options={'xatol': 1e-4, 'fatol': 1e-5, 'disp': True})
            print("Optimal t value: {:.4f}".format(res.x[0]))
            procedure = "Testing"
        else:
            if args.mlp_idx is None:
                raise ValueError("training needs --mlp_idx: the mapping MLP whose prediction conditions the noise estimator (-1: the ViT)")
            runner.train(mlp_idx=args.mlp_idx)                       # main.py:363-365
            procedure = "Training"
        logging.info("\n{} procedure finished. It took {:.4f} minutes.\n\n\n".format(procedure, (time.time() - start_time) / 60))
    except Exception:
        logging.error(traceback.format_exc())                     # main.py:377-378: logged, exit code stays 0 ...
        failed = True
    finally:
        nd_dist.shutdown()
        for handler in logger.handlers[:]:
            logger.removeHandler(handler)
            handler.close()
    # ... for a single process, as in the reference.  A rank of a multi-GPU run that failed must not look successful: its
    # peers would wait in the batch's all-gather until the RCCL timeout and torchrun would report rc 0.
    return 1 if (failed and world > 1) else 0


if __name__ == "__main__":
    sys.exit(main())
