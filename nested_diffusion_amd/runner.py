"""Mirror of the reference runner's inference path: class Diffusion of
diffusion/classification_train_separately.py -- __init__ schedule block (:215-226), conditioner
loading (:249-275), compute_guiding_prediction (:330-348), convert_to_prob (:392-398),
compute_ensemble_confidence (:425-447), majority_voting_for_mc_samples (:51-68) and the hot loop
of test_atk (:749-794), plus the report metrics and test_calibrate.  Three jobs of the reference's class live in modules of
their own and are only called from here: the rank's batch pipeline (upload.py), the robustness perturbations (perturb.py) and the
training loop of one noise estimator, train (:842-1141; train_diffusion.py).

Host code is PyTorch plumbing; every tensor operation of the hot path runs in libnd_hip.so.
"""
from __future__ import annotations

import logging
import os
import time
from typing import Dict, List, Optional, Sequence

import torch

from . import ops, perturb as P, upload
from .diffusion_utils import SKIP_TYPES, sampler_plan, schedule_tables, timestep_sequence
from .engine import EnsembleEngine
from .mapping import GuidingConditioner, load_checkpoint_object, load_conditioner, require_fp32_split
from . import dist as nd_dist

CHEST = ['ChestXRay', 'ChestXRayAtkFGSM', 'ChestXRayAtkPGD', 'ChestXRayAtkBIM', 'ChestXRayAtkAUTOPGD', 'ChestXRayAtkCW',
         'ChestXRayValidate']
ISIC = ['ISICSkinCancer', 'ISICSkinCancerAtkFGSM', 'ISICSkinCancerAtkPGD', 'ISICSkinCancerAtkBIM',
        'ISICSkinCancerAtkAUTOPGD', 'ISICSkinCancerAtkCW', 'ISICSkinCancerValidate']


def majority_voting_for_mc_samples(predictions: Sequence[torch.Tensor]) -> torch.Tensor:
    """classification_train_separately.py:51-68 -- mode over samples of argmax(raw y_0); ties -> smallest label."""
    samples = torch.stack([p if p.is_cuda else p.cuda() for p in predictions]).float()
    _, vote, _ = ops.aggregate(samples, 1.0)
    return vote.to(predictions[0].device)


def set_seed(seed) -> None:
    """:31-38, called from Diffusion.__init__ (:198): torch (CPU + every GPU), numpy and python `random`."""
    import random
    import numpy as np
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)


def temperature_for(dataset: str) -> float:
    """classification_train_separately.py:318-327."""
    if dataset in CHEST:
        return 0.1737
    if dataset in ISIC:
        return 0.3162
    raise NotImplementedError(dataset)


SAMPLE_TYPES = ("generalized", "ddpm_noisy")


def sampler_request(args) -> Optional[dict]:
    """--sample_steps N [--skip_type uniform|quadratic] [--sample_type generalized|ddpm_noisy] [--eta E] as {'steps', 'skip_type', 'eta'},
    or None when --sample_steps is not given: the other three are then not read at all, as in the reference, which declares them and
    never reads them, and the run does what it always did.  'ddpm_noisy' means eta = 1 (ancestral sampling on the sub-chain);
    'generalized' takes --eta (the reference's default 0.0: the deterministic chain).  Anything else is refused by name (ValueError):
    a pure host function, called before the GPU is touched."""
    steps = getattr(args, "sample_steps", None)
    if steps is None:
        return None
    skip_type, sample_type, eta = getattr(args, "skip_type", "uniform"), getattr(args, "sample_type", "generalized"), getattr(args, "eta", 0.0)
    if isinstance(steps, bool) or int(steps) != steps or steps < 1:
        raise ValueError(f"--sample_steps must be an integer >= 1 (got {steps!r})")
    if skip_type not in SKIP_TYPES:
        raise ValueError(f"--skip_type must be one of {SKIP_TYPES} (got {skip_type!r})")
    if sample_type not in SAMPLE_TYPES:
        raise ValueError(f"--sample_type must be one of {SAMPLE_TYPES} (got {sample_type!r})")
    eta = 1.0 if sample_type == "ddpm_noisy" else float(eta)
    if not 0.0 <= eta <= 1.0:
        raise ValueError(f"--eta must lie in [0, 1] (got {eta})")
    return {"steps": int(steps), "skip_type": skip_type, "eta": eta}


class Diffusion(object):
    def __init__(self, args, config, device=None, conditioner: Optional[GuidingConditioner] = None,
                 noise_estimator_states: Optional[List[Dict[str, torch.Tensor]]] = None):
        """`conditioner` / `noise_estimator_states` let synthetic runs (no checkpoints on disk) inject
        weights; otherwise they are read from the reference's checkpoint layout."""
        self.args, self.config = args, config
        self.seed = getattr(args, "seed", 0)
        if self.seed is not None:
            set_seed(self.seed)                                              # :198
        # operand dtype of the weight-streaming layers: --fp16 (or model.operand_dtype: f16 in the YAML) selects the fp16
        # mode of BASELINE config 5; the reference itself only has fp32
        self.operand_dtype = "f16" if getattr(args, "fp16", False) else getattr(config.model, "operand_dtype", "f32")
        if device is None:
            device = torch.device("cuda")
        self.device = torch.device(device)
        self.num_timesteps = config.diffusion.timesteps
        self.mc_trials = int(getattr(args, "mc_trials", 20) or 20)          # hard-coded 20 at :770
        tables = schedule_tables(config.diffusion.beta_schedule, self.num_timesteps, config.diffusion.beta_start, config.diffusion.beta_end)
        self.betas, self.alphas = tables.betas.to(self.device), tables.alphas.to(self.device)
        self.one_minus_alphas_bar_sqrt = tables.one_minus_alphas_bar_sqrt.to(self.device)
        # --sample_steps: a sampler plan over the schedule (diffusion_utils.sampler_plan; not a reference mode).  test_atk, test_calibrate,
        # predict_batch and ensemble_target run its S steps per chain; the validation sampling inside train() stays on the full chain,
        # whose accuracy is what picks the best checkpoint.  --timesteps is still the reference's override of diffusion.timesteps.
        self.use_sampler(sampler_request(args))
        self.temperature = temperature_for(config.data.dataset)
        self.selected_block_indices = [0, 1, 2, 3, 4]                       # :275
        if conditioner is None:
            if config.diffusion.aux_cls.arch != "sevit":
                raise NotImplementedError("only aux_cls.arch == 'sevit' is on the hot path")
            ds = "ChestXRay" if config.data.dataset in CHEST else "ISICSkinCancer"
            conditioner = load_conditioner(config.diffusion.trained_aux_cls_ckpt_path, ds, self.device, dtype=self.operand_dtype)
        self.cond_pred_model = conditioner
        self.num_noise_estimators_required = len(conditioner.mlps) + 1      # :274 (the +1 is never sampled, Q1)
        self._states = noise_estimator_states
        self.engine: Optional[EnsembleEngine] = None
        self.members: List[int] = []
        self.bytes_uploaded = 0          # image bytes this rank has sent over PCIe (its shard of every batch, nothing else)

    def use_sampler(self, request: Optional[dict]) -> None:
        """Sample with the plan of sampler_request's {'steps', 'skip_type', 'eta'} from here on, or (None) with every timestep again:
        self.plan, self.sample_steps = the reverse steps per chain, and the engine's plan if the noise estimators are loaded."""
        self.sampler, self.plan = request, None
        if request is not None:
            tau = timestep_sequence(self.num_timesteps, request["steps"], request["skip_type"])
            self.plan = sampler_plan(self.one_minus_alphas_bar_sqrt, tau, request["eta"])
        self.sample_steps = self.num_timesteps if self.plan is None else len(self.plan.timesteps)
        if getattr(self, "engine", None) is not None:
            self.engine.set_sampler(self.plan)

    # ---- conditioner -------------------------------------------------------------------------
    def compute_guiding_prediction(self, x, include_full_vit: bool = True):
        """:330-348."""
        return self.cond_pred_model.compute_guiding_prediction(x, include_full_vit)

    # ---- aggregation --------------------------------------------------------------------------
    def convert_to_prob(self, logits: torch.Tensor) -> torch.Tensor:
        """:392-398 -- softmax(-(y-1)^2 / T)."""
        dev = logits.device
        x = logits.float().to(self.device).reshape(1, -1, logits.shape[-1]).contiguous()
        _, _, probs = ops.aggregate(x, self.temperature, return_probs=True)
        return probs.reshape(logits.shape).to(dev)

    def compute_ensemble_confidence(self, outputs: List[torch.Tensor]) -> torch.Tensor:
        """:425-447 -- replaces every list entry by its probabilities (quirk Q4) and returns the mean."""
        dev = outputs[0].device
        samples = torch.stack([o.to(self.device) for o in outputs]).float().contiguous()
        prob, _, probs = ops.aggregate(samples, self.temperature, return_probs=True)
        for i in range(len(outputs)):
            outputs[i] = probs[i].to(dev)
        return prob.to(dev)

    # ---- noise estimators ---------------------------------------------------------------------
    def load_noise_estimators(self, max_batch: int, mc_trials: Optional[int] = None) -> None:
        """:684-697.  Members actually sampled are selected_block_indices ∩ available checkpoints
        (the reference asks for len(mlps)+1 paths and dies on the 6th, quirk Q1)."""
        cfg = self.config
        mc = mc_trials or self.mc_trials
        if self._states is None:
            self._states = self._read_noise_estimator_states()
        self.members = [i for i in self.selected_block_indices if i < len(self._states)]
        K = len(self.members)
        self.engine = EnsembleEngine(cfg.data.num_classes, cfg.model.data_dim, cfg.model.hidden_dim, cfg.model.feature_dim,
                                     self.num_timesteps, n_members=K, max_batch=max_batch, max_rows=max_batch * mc,
                                     device=self.device, dtype=self.operand_dtype)
        for slot, i in enumerate(self.members):
            self.engine.load_member(slot, self._states[i])
        self.engine.set_schedule(self.alphas, self.one_minus_alphas_bar_sqrt)
        if self.plan is not None:
            self.engine.set_sampler(self.plan)
        self._seeded_first = None
        self._seed_noise(0)            # in-library noise (predict_batch without a noise tensor)
        self._states = None            # device copies live in the engine

    def _read_noise_estimator_states(self) -> List[Dict[str, torch.Tensor]]:
        """:684-697: the 'noise_estimator' state_dicts of the config's checkpoints, in member order; with args.use_ema their 'ema'
        entries instead (the averaged weights a training run with --ema saved beside the live ones; a KeyError names the file that
        has none).  Every reader of the checkpoints goes through here: --test, --calib and ensemble_target."""
        paths = self.config.diffusion.trained_diffusion_ckpt_path[0]
        entry = "ema" if getattr(self.args, "use_ema", False) else "noise_estimator"
        states = []
        for i in range(min(len(paths), self.num_noise_estimators_required)):
            state = load_checkpoint_object(paths[i])      # {'noise_estimator': state_dict, 'optimizer': ..., 'epoch': ...} (:1120-1126)
            if entry not in state:
                raise KeyError(f"{paths[i]} holds no '{entry}' entry" + (": --use_ema needs a checkpoint written by a training run with --ema"
                                                                          if entry == "ema" else ""))
            states.append(state[entry])
            logging.info("Diffusion model %d loaded", i)
        return states

    def ensemble_target(self, mc: int = 1, members: Optional[Sequence[int]] = None, seed: Optional[int] = None):
        """The model of a white-box attack on the ensemble itself (ensemble_grad.EnsembleTarget) from this runner's conditioner, config,
        temperature and noise-estimator checkpoints: Attack(eps, 'PGD', runner.ensemble_target(mc=2)) is then what test_atk(attack=...)
        takes.  load_noise_estimators drops the host states once the engine holds them, so this call reads the checkpoints again; states
        that were injected (no checkpoints on disk) must still be there: build the target before the first test_atk.  The target holds
        its OWN packed copy of every selected member (the module docstring of ensemble_grad states the bytes)."""
        from .ensemble_grad import EnsembleTarget
        require_fp32_split("ensemble_target", dtype=self.operand_dtype)
        states = self._states
        if states is None:
            paths = getattr(self.config.diffusion, "trained_diffusion_ckpt_path", None)
            if not paths or not paths[0]:
                raise RuntimeError("the injected noise-estimator states are gone (load_noise_estimators dropped them) and the config names "
                                   "no checkpoints: call ensemble_target() before load_noise_estimators() / test_atk()")
            states = self._read_noise_estimator_states()
        if members is None:
            members = [i for i in self.selected_block_indices if i < len(states) and i < len(self.cond_pred_model.mlps)]
        plan = {} if self.sampler is None else {"sample_steps": self.sampler["steps"], "skip_type": self.sampler["skip_type"],
                                                "eta": self.sampler["eta"]}
        return EnsembleTarget(self.cond_pred_model, states, self.config, mc=mc, members=members, temperature=self.temperature,
                              seed=self.seed or 0 if seed is None else seed, **plan)

    def _seed_noise(self, first_image: int) -> None:
        """Seed the library's generator ONCE per (run, shard): nd_seed resets the device-side batch counter, so seeding again before
        every pass over the data (each Nelder-Mead evaluation of `--calib` under ND_CALIB_RESAMPLE=1, or test_atk after it) would
        replay identical noise.  Later passes just let the counter run on."""
        if self._seeded_first != first_image:
            self.engine.seed(self.seed or 0, first_image=first_image)
            self._seeded_first = first_image

    # ---- training of one noise estimator (:842-1141) ---------------------------------------------
    def train(self, mlp_idx: int, train_loader=None, valid_loader=None) -> dict:
        """Diffusion.train (:842-1141) for the noise estimator conditioned on mapping MLP `mlp_idx` (-1: on the full ViT's output), on ONE
        GPU: train_diffusion.train_request refuses before anything is built, train_diffusion.train_noise_estimator is the loop (its
        docstring says what a step, a validation, the best file, ckpt.pth and --ema are), with this runner's conditioner, schedule and
        seed.  The trainer stays reachable as self.trainer, also when the run is cut: its training_state() is what a snapshot holds.
        Returns {'losses': per-epoch last loss, 'accuracies': {epoch: acc}, 'best': path or None}."""
        from . import train_diffusion as td
        request = td.train_request(self.args, self.config, mlp_idx, len(self.cond_pred_model.mlps), self.operand_dtype)
        return td.train_noise_estimator(request, self.args, self.config, self.device, guide=self.compute_guiding_prediction,
                                        alphas=self.alphas, one_minus_alphas_bar_sqrt=self.one_minus_alphas_bar_sqrt, seed=self.seed or 0,
                                        train_loader=train_loader, valid_loader=valid_loader,
                                        built=lambda trainer: setattr(self, "trainer", trainer))

    # ---- the hot path (:749-794) --------------------------------------------------------------
    @torch.no_grad()
    def predict_batch(self, images_224: torch.Tensor, noise: Optional[torch.Tensor] = None, mc_trials: Optional[int] = None,
                      clone: bool = True, use_graph: bool = True):
        """images [B,3,224,224] on the GPU -> dict(samples [K*mc, B, C] raw y_0 member-major then trial,
        vote [B], prob [B, C], probs [K*mc, B, C], yhat [K, B, C]).  noise: optional [K, T, B*mc, C] in reference draw order
        (row = trial*B + image); None = drawn inside the library (the reference draws inside its loop, diffusion_utils.py:67,139).
        ONE library call: the conditioner (:753), the softmax (:755-758), the encoder hoist, the K x mc sampling loops
        (:767-777) and the aggregation (:786-789) are one hipGraph launch after the first batch of a shape."""
        if self.engine is None:
            raise RuntimeError("call load_noise_estimators() first")
        if self.members != list(range(len(self.members))) or len(self.members) > len(self.cond_pred_model.mlps):
            raise RuntimeError(f"member k is conditioned on mapping MLP k: the loaded noise estimators {self.members} must be "
                               f"0..K-1 with K <= {len(self.cond_pred_model.mlps)} mapping MLPs")
        mc = mc_trials or self.mc_trials
        eng, T = self.engine, self.sample_steps
        images_224 = ops._f32(images_224, "images")
        cond = self.cond_pred_model.handle(images_224.shape[0], images_224.shape[-1])
        return eng.predict_batch(cond, images_224, noise, mc, T, self.temperature, use_graph=use_graph, clone=clone)

    # ---- world-size independent randomness ---------------------------------------------------------
    def draw_noise(self, B_total: int, lo: int, hi: int, mc: Optional[int] = None) -> torch.Tensor:
        """torch-generator draws for rows [lo, hi) of a test batch of B_total images: [K, T, (hi-lo)*mc, C], for callers that want
        explicit noise; T = the steps per chain, S of a sampler plan (test_atk itself uses the library's generator, which has the same property at no cost).
        Every rank holds the same --seed (the reference's set_seed, :31-38), draws the draws of the WHOLE batch
        [K, T, mc, B_total, C] and keeps its own images, so image i sees the same K*T*mc draws at any world size
        (and rows of different ranks are not copies of each other)."""
        mc = mc or self.mc_trials
        K, T, C = len(self.members), self.sample_steps, self.config.data.num_classes
        z = torch.randn(K, T, mc, B_total, C, device=self.device)
        return z[:, :, :, lo:hi].reshape(K, T, mc * (hi - lo), C).contiguous()

    def _perturbs(self) -> bool:
        """Does any flag of the robustness protocol change the pixels on the device (perturb.requested: :726-737)?"""
        return bool(P.requested(self.args))

    def _rank_batches(self, test_loader, lo: int, hi: int, B_total: int):
        """The rank's slice of every batch of the loader, on the device: yields (images [hi-lo, 3, S, S] perturbed, targets [hi-lo]).
        upload.rank_batches is the pipeline (pinned staging, a side stream, straight into the library's input buffer when nothing
        perturbs or attacks the batch on the device); this runner's engine, perturb and bytes_uploaded are what it works on."""
        def count(n):
            self.bytes_uploaded += n

        direct_ok = not self._perturbs() and getattr(self, "_attack", None) is None   # an attack reads the batch while the next one uploads
        yield from upload.rank_batches(test_loader, lo, hi, B_total, device=self.device, engine=self.engine, direct_ok=direct_ok,
                                       perturb=self.perturb, mc_trials=self.mc_trials, sample_steps=self.sample_steps, count=count)

    # ---- temperature calibration (:449-629, driven by main.py:356-361) ---------------------------
    def test_calibrate(self, temp=None, test_loader=None):
        """ECE of the ensemble at scaling temperature `temp` on the validation set (:449-629).  The reference
        re-runs the whole sampler for every temperature the Nelder-Mead search tries although the samples y_0 do not
        depend on it; here the raw samples are drawn once and cached (set ND_CALIB_RESAMPLE=1 for the as-written,
        stochastic objective), so each further evaluation is one aggregation + one calibration-error kernel."""
        if temp is not None:
            self.temperature = float(temp[0] if hasattr(temp, "__len__") else temp)
        resample = bool(int(os.environ.get("ND_CALIB_RESAMPLE", "0")))
        if resample or getattr(self, "_calib_cache", None) is None:
            rank, world = nd_dist.rank_world()
            B = self.config.testing.batch_size
            lo, hi = nd_dist.shard_bounds(B, rank, world)
            if test_loader is None:
                from .data import get_test_loader
                test_loader = get_test_loader(self.args, self.config, shard=(lo, hi) if world > 1 else None)
            if self.engine is None:
                self.load_noise_estimators(max_batch=max(hi - lo, 1))
            self._seed_noise(lo)
            samples, targets = [], []
            for images, target in self._rank_batches(test_loader, lo, hi, B):
                out = self.predict_batch(images)
                S = out["samples"].shape[0]
                flat = out["samples"].permute(1, 0, 2).reshape(hi - lo, -1)                      # [B_local, S*C]
                flat = torch.cat([flat, target.to(torch.float32)[:, None]], dim=1).contiguous()  # + the rows' targets
                flat = nd_dist.all_gather_rows(flat, B, world)
                samples.append(flat[:, :-1].reshape(B, S, -1).permute(1, 0, 2).contiguous())
                targets.append(flat[:, -1].to(torch.int64))
            self._calib_cache = (torch.cat(samples, dim=1).contiguous(), torch.cat(targets))
        samples, targets = self._calib_cache
        prob, vote, _ = ops.aggregate(samples, self.temperature)              # compute_ensemble_confidence (:612)
        rep = ops.report(prob, prob, prob, vote, targets, self.temperature, n_bins=10)   # compute_ece (:619)
        ece = float(rep["ece"])
        print(f"Ours ECE: {ece} \n")
        logging.info(f"Ours ECE: {ece} \n")
        return ece

    # ---- input perturbations (:726-737), in the reference's order ------------------------------
    def perturb(self, images_224: torch.Tensor, lo: int = 0, hi: Optional[int] = None, B_total: Optional[int] = None) -> torch.Tensor:
        """perturb.apply with this run's flags: rows [lo, hi) of a test batch of B_total images (default: the whole batch), the random
        calls made for the WHOLE batch."""
        return P.apply(self.args, images_224, lo, hi, B_total)

    # ---- test loop ----------------------------------------------------------------------------
    def test_atk(self, test_loader=None, attack=None):
        """:631-840: input perturbations (:726-737), the hot path, and the report the reference prints (accuracy, ECE,
        per-class PIW and variances, :801-838).  attack: an attack.Attack, L2Attack or CarliniWagner (attack.make_attack), a square.SquareAttack or an autoattack.AutoAttack (AUTOPGD) applied to this rank's
        rows after the perturbations (:738-739; the random start of image i is keyed on its global index).  The --attack_name switch itself still raises."""
        args, config = self.args, self.config
        if getattr(args, "attack_name", None) not in (None, "None"):
            raise NotImplementedError("adversarial attacks need gradients through the ViT: out of scope")
        rank, world = nd_dist.rank_world()
        B = config.testing.batch_size
        lo, hi = nd_dist.shard_bounds(B, rank, world)
        if test_loader is None:
            from .data import get_test_loader
            test_loader = get_test_loader(args, config, shard=(lo, hi) if world > 1 else None)   # each rank decodes its own rows only
        self.load_noise_estimators(max_batch=max(hi - lo, 1))
        # the sampler's draws come from the library's counter-based generator keyed on the GLOBAL image index (lo = this rank's
        # first image) and the batch counter: image i sees the same K*T*mc draws at any world size
        self._seed_noise(lo)
        mv_class, target_class, prob_mc, piw_mc, var_mc = [], [], [], [], []
        n_step_img, t0 = 0, time.time()
        self._attack = attack
        for n_batch, (images, target) in enumerate(self._rank_batches(test_loader, lo, hi, B)):   # :715-737, this rank's rows only
            if attack is not None:                                           # :738-739
                from .attack import apply_attack
                images = apply_attack(attack, images, target, attack.attack_type, first_image=n_batch * B + lo)
            out = self.predict_batch(images, clone=False)
            # spread of the K*mc per-sample probabilities per image (what the reference keeps in pred_mc, quirk Q4)
            piw, var = ops.sample_stats(out["probs"])
            packed = torch.cat([out["prob"], piw, var, out["vote"].to(torch.float32)[:, None], target.to(torch.float32)[:, None]], dim=1)
            packed = nd_dist.all_gather_rows(packed, B, world)               # the single RCCL all-gather of a batch
            C = out["prob"].shape[1]
            prob_mc.append(packed[:, :C]); piw_mc.append(packed[:, C:2 * C]); var_mc.append(packed[:, 2 * C:3 * C])
            mv_class.append(packed[:, 3 * C].to(torch.int64)); target_class.append(packed[:, 3 * C + 1].to(torch.int64))
            n_step_img += B * len(self.members) * self.mc_trials * self.sample_steps      # the steps that ran: S of a plan, else T
        torch.cuda.synchronize(self.device)
        dt = time.time() - t0
        if self.engine.loop_form() == "one_launch":
            self.engine.persist_status()                                     # raises if a barrier wait of the one-launch loop was abandoned
        rep = ops.report(torch.cat(piw_mc), torch.cat(var_mc), torch.cat(prob_mc), torch.cat(mv_class), torch.cat(target_class),
                         self.temperature, n_bins=10)                        # :801-815
        acc = rep["accuracy"]
        if rank == 0:
            msg = (f"Majority voting accuracy for MC: {rep['accuracy'] :.4f} \n" +
                   f"ECE: {rep['ece'] :.4f} \n" +
                   f"Average correct PIW per class: {rep['piw_correct']} \n" +
                   f"Average incorrect PIW per class: {rep['piw_incorrect']} \n" +
                   f"Average correct variances per class: {rep['var_correct']} \n" +
                   f"Average incorrect variances per class: {rep['var_incorrect']}")
            print(msg)                                                       # :820-825
            logging.info(msg + " \n")                                        # :829-838
            logging.info("throughput: %.1f denoising-step*images/s over %d GPU(s)", n_step_img / max(dt, 1e-9), world)
        self.last_report = rep
        self.last_probs = torch.cat(prob_mc)
        return acc
