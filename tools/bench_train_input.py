"""The training input of a mapping-MLP run at config dims (ViT-B/16 prefix, 150528 -> 4096 Classifier, batches of 30) on a seeded tree
of 600 JPEGs of 1024 x 1024: what an epoch costs when a DataLoader decodes every image, when the batches are gathered from the
device-resident set (data.DeviceImageSet), and with no input work at all.  GPU only.

    python tools/bench_train_input.py [--mode all|loader|device] [--root DIR] [--images 600] [--side 1024] [--batch 30] [--epochs 1]
                                      [--loader_json FILE ...] [--out profiles/train_input_bench.json]

  (a) --mode loader   epoch wall time of MappingTrainer.train_epoch fed by make_loaders(root, dataset, preprocess, batch, seed).  This
                      mode uses only that five-argument signature and nothing of the device set, so the same file runs on a commit from
                      before the device set; such runs' output files are handed to a later run with --loader_json and recorded beside it.
  (b) --mode device   the same epoch from make_loaders(..., cache='device');
  (c)                 the same epoch from pre-made device tensors, three times, for the spread;
  (d)                 the one-off build of the store at 16 decode threads (and the upload);
  (e)                 one nd_img_gather_u8 launch by device events (a window of launches between two events), with its bytes, and one
                      whole DeviceImageSet.batch call (index check, upload, allocation, launch) by the wall clock.
--root keeps the tree between runs (it is written only if absent); without it the tree lives in a temporary directory.
Prints one JSON line (and writes it to --out).  Times in seconds unless the key says otherwise; what a mode does not measure is the
string 'not measured'."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nested_diffusion_amd import synthetic  # noqa: E402
from nested_diffusion_amd.mapping import VisionTransformer  # noqa: E402
from nested_diffusion_amd.train_mapping import MappingTrainer, make_loaders  # noqa: E402

NOT = "not measured"
DATASET, PREPROCESS, SEED = "ChestXRay", "grayscaled", 3


def write_tree(root: str, n_images: int, side: int) -> None:
    """<root>/{training,validation}/{NORMAL,PNEUMONIA}/: n_images JPEGs of side x side under training (half per class), two under
    validation.  Seeded per file (16 threads write them): a smooth field plus noise, so that the files have the size and the decode
    cost of photographs."""
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    yy, xx = np.mgrid[0:side, 0:side].astype(np.float32) / side
    jobs = []
    for split, n in (("training", n_images), ("validation", 2)):
        for ci, cls in enumerate(("NORMAL", "PNEUMONIA")):
            d = os.path.join(root, split, cls)
            os.makedirs(d)
            jobs += [(os.path.join(d, f"{i:04d}.jpg"), ci, 1234 + len(jobs) + i) for i in range(n // 2)]

    def one(job):
        path, ci, seed = job
        rng = np.random.RandomState(seed)
        f = rng.uniform(1, 6, 3)
        field = 110 + 70 * np.sin(6.28 * (f[0] * xx + f[1] * yy)) * np.cos(6.28 * f[2] * yy) + 30 * ci
        a = np.clip(field[:, :, None] + rng.normal(0, 12, (side, side, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(a, "RGB").save(path, quality=90)

    with ThreadPoolExecutor(max_workers=16) as pool:
        list(pool.map(one, jobs))


def epoch(tr, loader) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.train_epoch(loader)                                   # ends with a read-back of the loss: the device is idle when it returns
    return time.perf_counter() - t0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=["all", "loader", "device"])
    ap.add_argument("--root", default=None)
    ap.add_argument("--images", type=int, default=600)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=30)
    ap.add_argument("--epochs", type=int, default=1, help="epochs timed per loader (the median is reported, all are listed)")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--loader_json", nargs="*", default=[], help="outputs of --mode loader runs made elsewhere (an earlier commit)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_input needs the GPU: there is nothing to measure without one")
    dev, B = "cuda", a.batch
    tmp = None
    root = a.root
    if root is None:
        tmp = tempfile.TemporaryDirectory(prefix="train_input_")
        root = os.path.join(tmp.name, "tree")
    if not os.path.isdir(root):
        t0 = time.perf_counter()
        write_tree(root, a.images, a.side)
        print(f"wrote {a.images} JPEGs of {a.side} x {a.side} under {root} in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    vit = VisionTransformer(synthetic.vit_state(seed=7, device=dev), 12, dev)
    tr = MappingTrainer(vit, 0, num_classes=2, lr=1e-3, seed=0)
    warm = synthetic.images(B, device=dev)
    for _ in range(3):                                       # the kernels' first launches, at the epoch's batch
        tr.step(warm, torch.arange(B) % 2)
    torch.cuda.synchronize()
    res = {"tool": "bench_train_input", "mode": a.mode, "images": a.images, "side": a.side, "batch": B, "steps_per_epoch": -(-a.images // B),
           "epoch_loader_s": NOT, "epoch_loader_all_s": NOT, "epoch_device_s": NOT, "epoch_device_all_s": NOT, "epoch_premade_s": NOT,
           "epoch_premade_min_max_s": NOT, "device_minus_premade_s": NOT, "build_s": NOT, "build_workers": NOT, "upload_s": NOT,
           "store_mb": NOT, "src_channels": NOT, "gather_us": NOT, "gather_us_min_max": NOT, "gather_mb_out": NOT, "gather_mb_in": NOT,
           "gather_tbps": NOT, "batch_call_us": NOT, "epoch_loader_parent_s": NOT, "epoch_loader_parent_all_s": NOT, "loader_over_device": NOT}
    if a.mode in ("all", "loader"):
        train, _ = make_loaders(root, DATASET, PREPROCESS, B, SEED)
        ts = [epoch(tr, train) for _ in range(a.epochs)]
        res["epoch_loader_s"], res["epoch_loader_all_s"] = round(statistics.median(ts), 4), [round(t, 4) for t in ts]
    if a.mode in ("all", "device"):
        from nested_diffusion_amd import _lib, data
        ds = data.ImageFolderDataset(os.path.join(root, "training"), DATASET, PREPROCESS)
        t0 = time.perf_counter()
        store, _ = data.build_store(ds, workers=16)
        res["build_s"], res["build_workers"] = round(time.perf_counter() - t0, 3), 16
        res["store_mb"], res["src_channels"] = round(store.nbytes / 1e6, 2), int(store.shape[1])
        del store
        with tempfile.TemporaryDirectory(prefix="train_input_cache_") as cache_dir:
            make_loaders(root, DATASET, PREPROCESS, B, SEED, cache="device", cache_dir=cache_dir, workers=16)      # writes the files
            t0 = time.perf_counter()
            train, _ = make_loaders(root, DATASET, PREPROCESS, B, SEED, cache="device", cache_dir=cache_dir, workers=16)
            torch.cuda.synchronize()
            res["upload_s"] = round(time.perf_counter() - t0, 3)             # both splits read from their files and uploaded
        ts = [epoch(tr, train) for _ in range(a.epochs)]
        res["epoch_device_s"], res["epoch_device_all_s"] = round(statistics.median(ts), 4), [round(t, 4) for t in ts]
        premade = [(x, y) for x, y in train]
        tp = [epoch(tr, premade) for _ in range(3)]
        res["epoch_premade_s"], res["epoch_premade_min_max_s"] = round(statistics.median(tp), 4), [round(min(tp), 4), round(max(tp), 4)]
        res["device_minus_premade_s"] = round(res["epoch_device_s"] - res["epoch_premade_s"], 4)
        del premade
        # (e) the launch alone
        dset = train.image_set
        H, W = dset.size
        idx = torch.randperm(len(dset), generator=torch.Generator().manual_seed(1))[:B]
        idx_dev, out = idx.to(torch.int32).to(dev), torch.empty(B, 3, H, W, device=dev)
        L, st = _lib.load(), _lib.current_stream_ptr()

        def launch():
            _lib.check(L.nd_img_gather_u8(dset.store.data_ptr(), len(dset), dset.store.shape[1], H * W, idx_dev.data_ptr(), B, dset.lut.data_ptr(),
                                          out.data_ptr(), st), "nd_img_gather_u8")

        for _ in range(10):
            launch()
        torch.cuda.synchronize()
        windows = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                launch()
            e1.record()
            torch.cuda.synchronize()
            windows.append(e0.elapsed_time(e1) / a.reps * 1e3)
        us = statistics.median(windows)
        mb_out, mb_in = out.numel() * 4 / 1e6, B * dset.store.shape[1] * H * W / 1e6
        res.update(gather_us=round(us, 2), gather_us_min_max=[round(min(windows), 2), round(max(windows), 2)], gather_mb_out=round(mb_out, 2),
                   gather_mb_in=round(mb_in, 2), gather_tbps=round((mb_out + mb_in) / us, 3))
        assert torch.equal(out, dset.batch(idx)[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            dset.batch(idx)
        torch.cuda.synchronize()
        res["batch_call_us"] = round((time.perf_counter() - t0) / a.reps * 1e6, 1)
    parent = []
    for path in a.loader_json:
        with open(path) as f:
            parent += json.loads([l for l in f.read().splitlines() if l.startswith("{")][-1])["epoch_loader_all_s"]
    if parent:
        res["epoch_loader_parent_s"], res["epoch_loader_parent_all_s"] = round(statistics.median(parent), 4), parent
    base = res["epoch_loader_parent_s"] if parent else res["epoch_loader_s"]
    if base != NOT and res["epoch_device_s"] != NOT:
        res["loader_over_device"] = round(base / res["epoch_device_s"], 1)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if tmp is not None:
        tmp.cleanup()
    return 0


if __name__ == "__main__":
    sys.exit(main())
