"""What one training snapshot of a noise estimator costs at the config's dimensions (data_dim 150528, hidden_dim = feature_dim = 4096:
about 8.2 GB on disk): the wall time of writing it (NoiseEstimatorTrainer.training_state + snapshot.atomic_save), the wall time of a
resume load (snapshot.read + load_training_state), and the peak device memory either adds to the resident model.

    python tools/bench_snapshot.py [--out profiles/snapshot_bench.json] [--dir <scratch directory>] [--dims D H F]

One condition is checked (exit 1 if it fails): while the snapshot is taken the device holds at most ONE row-major weight beside the
model -- encoder_x.0.weight, H x D x 4 bytes -- read with torch.cuda.max_memory_allocated.  The times are recorded, not gated: they are
mostly the host's memory copies and its disk.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nested_diffusion_amd import snapshot                                         # noqa: E402
from nested_diffusion_amd.train_diffusion import NoiseEstimatorTrainer            # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--dir", default=None, help="directory for the snapshot file (default: a temporary one, removed afterwards)")
    ap.add_argument("--dims", type=int, nargs=3, default=(150528, 4096, 4096), metavar=("D", "H", "F"))
    args = ap.parse_args()
    D, H, F = args.dims
    C, T, B = 2, 1000, 4
    ns = argparse.Namespace
    cfg = ns(data=ns(num_classes=C), model=ns(data_dim=D, hidden_dim=H, feature_dim=F, arch="linear"),
             diffusion=ns(timesteps=T, beta_schedule="linear", beta_start=1e-4, beta_end=0.02, include_guidance=True),
             optim=ns(optimizer="Adam", lr=1e-3, beta1=0.9, eps=1e-8, weight_decay=0.0, amsgrad=False, grad_clip=1.0))
    dev = torch.device("cuda")
    trainer = NoiseEstimatorTrainer(cfg, dev, seed=0)
    # no step is taken: Adam's moments are zero, which changes neither the bytes moved nor the file's size (torch.save does not compress)
    trainer.run_meta = {"mlp_idx": 0, "dataset": "ChestXRay", "batch_size": B, "train_batches": 1, "epochs": 1}
    torch.cuda.synchronize()
    print(f"trainer at D={D} H={H} F={F}: {torch.cuda.memory_allocated() / 1e9:.2f} GB resident", flush=True)
    one_tensor = H * D * 4
    scratch = args.dir or tempfile.mkdtemp(prefix="nd_snapshot_")
    path = os.path.join(scratch, "ckpt.pth")
    try:
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        state = trainer.training_state()
        t1 = time.perf_counter()
        snapshot.atomic_save({"trainer": state, "loop": {"next_epoch": 1}, "rng": snapshot.rng_state(dev, None)}, path)
        t2 = time.perf_counter()
        snap_extra = torch.cuda.max_memory_allocated() - base
        size = os.path.getsize(path)
        del state
        print(f"snapshot: {t2 - t0:.1f} s ({t1 - t0:.1f} s off the device, {t2 - t1:.1f} s to disk), {size / 1e9:.2f} GB, "
              f"peak extra device memory {snap_extra / 1e9:.3f} GB", flush=True)
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t3 = time.perf_counter()
        snap = snapshot.read(path)
        t4 = time.perf_counter()
        trainer.load_training_state(snap["trainer"])
        torch.cuda.synchronize()
        t5 = time.perf_counter()
        load_extra = torch.cuda.max_memory_allocated() - base
        print(f"resume load: {t5 - t3:.1f} s ({t4 - t3:.1f} s from disk, {t5 - t4:.1f} s onto the device), peak extra device memory "
              f"{load_extra / 1e9:.3f} GB", flush=True)
    finally:
        if args.dir is None:
            shutil.rmtree(scratch, ignore_errors=True)
        elif os.path.exists(path):
            os.unlink(path)
    ok = snap_extra <= one_tensor
    res = {"what": "noise-estimator training snapshot", "data_dim": D, "hidden_dim": H, "feature_dim": F, "file_gb": round(size / 1e9, 3),
           "snapshot_s": round(t2 - t0, 2), "snapshot_device_to_host_s": round(t1 - t0, 2), "snapshot_write_s": round(t2 - t1, 2),
           "resume_load_s": round(t5 - t3, 2), "resume_read_s": round(t4 - t3, 2), "resume_host_to_device_s": round(t5 - t4, 2),
           "one_tensor_gb": round(one_tensor / 1e9, 3), "snapshot_peak_extra_device_gb": round(snap_extra / 1e9, 3),
           "resume_peak_extra_device_gb": round(load_extra / 1e9, 3), "one_tensor_bound_holds": bool(ok),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        print(f"FAILED: the snapshot added {snap_extra} bytes of device memory, above one row-major weight ({one_tensor})", file=sys.stderr)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
