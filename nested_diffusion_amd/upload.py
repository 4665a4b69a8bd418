"""The rank's batch pipeline of the test and calibration loops (runner.Diffusion._rank_batches): host batches of a loader, sliced to the
rank's rows, pinned, and copied to the device on a side stream while the previous batch is still being sampled.  Host code: PyTorch
streams and events around the engine's input buffer; no kernel of its own."""
from __future__ import annotations

import numpy as np
import torch


def rank_batches(loader, lo: int, hi: int, B_total: int, *, device, engine, direct_ok: bool, perturb, mc_trials: int, sample_steps: int,
                 count):
    """The rank's slice of every batch of the loader, on the device: yields (images [hi-lo, 3, S, S] perturbed, targets [hi-lo]).
    A loader that is already sharded (data.get_test_loader(shard=...): its .shard attribute) hands over the rank's rows only -- only
    those files were decoded; a full-batch loader (the reference's, or a caller's) is sliced on the HOST.  The slice is pinned
    (as handed over, or through a staging buffer) and copied on a side stream, never on the compute stream
    (classification_train_separately.py:722 is a blocking .to(device) of the whole batch on the compute stream):
      * no device-side perturbation configured: STRAIGHT into the library's input buffer, as soon as the previous batch's graph has
        read that buffer (nd_set_input_flag: about a quarter into the batch) -- the transfer runs beside the previous batch's sampler,
        with no staging buffer on the device and no device-to-device copy;
      * otherwise: into one of two device buffers one batch ahead (perturb then makes new tensors out of it).
    direct_ok: the caller allows the first path (no perturbation flag, no attack set); it is taken for 4-D host batches when there is
    an `engine` (mc_trials and sample_steps name its input buffer).  perturb(images, lo, hi, B_total) is applied on the second path;
    count(n) is told the image bytes of every host-to-device copy."""
    main = torch.cuda.current_stream(device)
    side = torch.cuda.Stream(device)
    sharded = getattr(loader, "shard", None) == (lo, hi)
    pins, bufs, evs, held = [None, None], [None, None], [None, None], [None, None]
    tpins, tbufs = [None, None], [None, None]

    def rows_of(item):
        images_raw, target = item
        x = images_raw if sharded else images_raw[lo:hi]
        t = target if sharded else target[lo:hi]
        if x.shape[0] != hi - lo:
            raise ValueError(f"loader handed {x.shape[0]} rows for the shard [{lo}, {hi})")
        return x, t

    def host_stage(k, x, t):
        """pinned source of the batch's H2D copy (the tensor itself if the loader pinned it) and of its targets"""
        if evs[k] is not None:
            evs[k].synchronize()                        # the copy that last read staging buffer k (two batches ago)
        if x.dtype == torch.float32 and x.is_pinned():  # a loader with pin_memory=True: nothing to stage
            src = x
        else:
            if pins[k] is None or pins[k].shape != x.shape:
                pins[k] = torch.empty(x.shape, dtype=torch.float32, pin_memory=True)
            if x.dtype == torch.float32 and x.is_contiguous():
                # one memcpy on this thread.  (Tensor.copy_ spreads a 19 MB copy over every logical CPU the box shows; under a
                # container's CPU quota that takes 20-60 ms instead of 2 -- measured: bench.py's pcie_inclusive leg)
                np.copyto(pins[k].numpy(), x.numpy())
            else:
                pins[k].copy_(x)
            src = pins[k]
        # the targets ride along (pinned too: a pageable H2D copy on the compute stream would hold the HOST until the running batch
        # has finished, and the launches behind it would start late)
        if tpins[k] is None or tpins[k].shape != t.shape or tpins[k].dtype != t.dtype:
            tpins[k] = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            tbufs[k] = torch.empty(t.shape, dtype=t.dtype, device=device)
        tpins[k].copy_(t)
        held[k] = src                                   # a caller's pinned batch stays alive until its copy has been waited for
        return src

    def side_copy(k, dst, src):
        """batch k's images into dst and its targets into tbufs[k] on the side stream; evs[k] is recorded behind both"""
        with torch.cuda.stream(side):
            dst.copy_(src, non_blocking=True)
            tbufs[k].copy_(tpins[k], non_blocking=True)
            evs[k] = torch.cuda.Event()
            evs[k].record(side)
        count(src.numel() * 4)

    first = None
    it = iter(loader)
    for first in it:
        break
    if first is None:
        return
    x0, _ = rows_of(first)
    if (not x0.is_cuda) and direct_ok and engine is not None and x0.dim() == 4:
        engine.enable_input_flag()
        fixed = engine.batch_buffers(hi - lo, mc_trials, sample_steps, tuple(x0.shape[1:]))["images"]
        k, item = 0, first
        while item is not None:
            x, t = rows_of(item)
            src = host_stage(k, x, t)
            engine.inputs_consumed()                    # every batch launched so far has read `fixed`
            side_copy(k, fixed, src)
            main.wait_event(evs[k])
            tdev = tbufs[k]
            k ^= 1
            yield fixed, tdev
            item = next(it, None)
        return

    def stage(k, item):
        x, t = rows_of(item)
        if x.is_cuda:                                   # a caller's loader that already lives on the device
            return x.to(device, torch.float32), t.to(device), None
        if bufs[k] is None or bufs[k].shape != x.shape:
            bufs[k] = torch.empty(x.shape, dtype=torch.float32, device=device)
        src = host_stage(k, x, t)
        side.wait_stream(main)                          # bufs[k]'s last reader (batch n - 1, already enqueued) before it is overwritten
        side_copy(k, bufs[k], src)
        return bufs[k], tbufs[k], evs[k]

    def finish(staged):
        x, t, ev = staged
        if ev is not None:
            main.wait_event(ev)
        return perturb(x, lo, hi, B_total), t

    nxt = stage(0, first)
    k = 1
    for item in it:
        cur, nxt = nxt, stage(k, item)
        k ^= 1
        yield finish(cur)
    yield finish(nxt)
