"""Loaders: the reference's disk layout (ImageFolder + Grayscale/Resize/ToTensor,
dataset_helper/chest_x_ray_dataset.py; host-side decode with PIL, as torchvision does), a synthetic loader
of the same tensor contract: batches (images [B,3,224,224] float32, target [B] int64), and the training side's device-resident
set (DeviceImageSet: decoded once, held on the GPU as bytes, batches gathered by one HIP launch in the DataLoader's order)."""
from __future__ import annotations

import os

import torch


class SyntheticLoader:
    """shard = (lo, hi): yield only rows [lo, hi) of every global batch (a rank's slice; the generator still runs over the whole
    batch, so row i holds the same pixels at any world size)."""

    def __init__(self, n_batches: int, batch_size: int, num_classes: int, seed: int = 1234, size: int = 224, shard=None):
        self.n, self.B, self.C, self.seed, self.size = n_batches, batch_size, num_classes, seed, size
        self.shard = tuple(shard) if shard is not None else None
        self.global_batch = batch_size

    def __len__(self):
        return self.n

    def __iter__(self):
        g = torch.Generator().manual_seed(self.seed)
        lo, hi = self.shard if self.shard is not None else (0, self.B)
        for _ in range(self.n):
            x = torch.rand(self.B, 3, self.size, self.size, generator=g)
            t = torch.randint(0, self.C, (self.B,), generator=g)
            yield (x, t) if self.shard is None else (x[lo:hi].contiguous(), t[lo:hi].contiguous())


class ShardBatchSampler:
    """Batch sampler of ONE rank: for every global batch b of `batch_size` consecutive samples (shuffle=False, drop_last=True:
    classification_train_separately.py:675-681, quirk Q12) the indices of its rows [lo, hi) only -- the rank decodes, pins and
    uploads its own slice of each batch and nothing else.  (lo, hi) = (0, batch_size) is the reference's loader."""

    def __init__(self, n_samples: int, batch_size: int, lo: int, hi: int):
        if not (0 <= lo <= hi <= batch_size):
            raise ValueError(f"shard [{lo}, {hi}) outside the batch of {batch_size}")
        self.n, self.B, self.lo, self.hi = int(n_samples), int(batch_size), int(lo), int(hi)

    def __len__(self):
        return self.n // self.B

    def __iter__(self):
        for b in range(self.n // self.B):
            yield list(range(b * self.B + self.lo, b * self.B + self.hi))


IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")   # torchvision.datasets.folder
PRECAL = {"ChestXRay": ((0.5094, 0.5234, 0.5289), (0.2189, 0.2225, 0.2244)),          # chest_x_ray_dataset.py:73-74
          "ISICSkinCancer": ((0.7187, 0.5684, 0.5464), (0.1212, 0.1325, 0.1434))}      # :139-140


class ImageFolderDataset(torch.utils.data.Dataset):
    """torchvision.datasets.ImageFolder semantics (classes = sorted sub-directories, samples sorted by path, RGB
    loader) followed by the reference's test-time transforms (dataset_helper/chest_x_ray_dataset.py:31-51, 76-96):
      grayscaled:   Grayscale(num_output_channels=3) -> Resize((224, 224)) -> ToTensor
      standardized: Resize((224, 224)) -> ToTensor -> Normalize(pre-calculated mean, std)
      attacked:     Resize((224, 224)) -> ToTensor (data_loader_attacks, :197-227: the adversarial PNG trees, already in [0, 1] RGB)
    written with the PIL calls torchvision makes for PIL inputs (L conversion, BILINEAR resize, /255)."""

    def __init__(self, root: str, dataset_name: str, preprocess: str, image_size=(224, 224)):
        from PIL import Image  # noqa: F401  (fail early if absent)
        if not os.path.isdir(root):
            raise FileNotFoundError(f"dataset directory not found: {root}")
        if preprocess not in ("grayscaled", "standardized", "attacked"):
            raise ValueError("Invalid preprocess type")
        if preprocess != "attacked" and dataset_name not in PRECAL:
            raise ValueError("Dataset name is not valid")
        self.classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
        if not self.classes:
            raise FileNotFoundError(f"Couldn't find any class folder in {root}.")
        self.class_to_idx = {c: i for i, c in enumerate(self.classes)}
        self.samples = []
        for c in self.classes:
            for d, _, files in sorted(os.walk(os.path.join(root, c), followlinks=True)):
                for f in sorted(files):
                    if f.lower().endswith(IMG_EXTENSIONS):
                        self.samples.append((os.path.join(d, f), self.class_to_idx[c]))
        self.root, self.preprocess, self.size = root, preprocess, tuple(image_size)
        if preprocess != "attacked":
            self.mean, self.std = (torch.tensor(v).view(3, 1, 1) for v in PRECAL[dataset_name])

    def __len__(self):
        return len(self.samples)

    def load_u8(self, i):
        """(uint8 ndarray [3, H, W], target): sample i decoded, converted and resized -- everything of __getitem__ before ToTensor.  With
        byte_table() this is the whole per-sample state (none of the reference's training transforms is random)."""
        import numpy as np
        from PIL import Image
        path, target = self.samples[i]
        with open(path, "rb") as f:
            img = Image.open(f).convert("RGB")                                  # default_loader / pil_loader
        if self.preprocess == "grayscaled":
            g = np.array(img.convert("L"), dtype=np.uint8)                      # F.to_grayscale(img, 3)
            img = Image.fromarray(np.dstack([g, g, g]), "RGB")
        img = img.resize(self.size[::-1], Image.BILINEAR)                       # Resize((h, w)) on a PIL image
        return np.ascontiguousarray(np.array(img, dtype=np.uint8).transpose(2, 0, 1)), target

    def _to_float(self, x: torch.Tensor) -> torch.Tensor:
        """ToTensor's /255 and, for standardized, Normalize, on a uint8 tensor [3, ...] with two trailing axes."""
        x = x.float().div(255)                                                  # ToTensor
        if self.preprocess == "standardized":
            x = (x - self.mean) / self.std                                      # Normalize
        return x

    def byte_table(self) -> torch.Tensor:
        """float32 [3, 256]: what __getitem__ makes of byte value v in channel c, by the same tensor expressions (each is one correctly
        rounded operation per element, so a table entry has the bits of the pixel)."""
        return self._to_float(torch.arange(256, dtype=torch.uint8).view(1, 256, 1).repeat(3, 1, 1)).view(3, 256).contiguous()

    def __getitem__(self, i):
        a, target = self.load_u8(i)
        return self._to_float(torch.from_numpy(a)), target


# ---- device-resident training sets: decode once, keep the bytes on the GPU, gather every batch with one launch (nd_img_gather_u8) ------
STORE_FORMAT = 1
MAX_WORKERS = 16                  # a command on the GPU machines may use 16 CPUs; os.cpu_count() shows the whole machine's
UPLOAD_CHUNK = 64 << 20           # bytes per host -> device copy of the store
CACHE_CHOICES = ("none", "device")   # the trainers' --cache / --train_cache


def cache_file(cache_dir, split: str, ds):
    """<cache_dir>/<split>_<preprocess>_<H>x<W>.npz, or None without a cache_dir."""
    return os.path.join(cache_dir, f"{split}_{ds.preprocess}_{ds.size[0]}x{ds.size[1]}.npz") if cache_dir else None


def _workers(workers) -> int:
    if workers is None:
        return min(MAX_WORKERS, len(os.sched_getaffinity(0)))
    workers = int(workers)
    if not 1 <= workers <= MAX_WORKERS:
        raise ValueError(f"workers must be in [1, {MAX_WORKERS}] (workers={workers})")
    return workers


def build_store(dataset, workers=None):
    """(store uint8 ndarray [N, Cs, H, W], targets int64 ndarray [N]): every sample's load_u8, decoded by a pool of `workers` threads
    (Pillow releases the GIL in decode, convert and resize).  Cs = 1 when the three planes of EVERY image are equal (checked here, image
    by image; always so for 'grayscaled'), else 3."""
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor
    workers, n = _workers(workers), len(dataset)
    if n < 1:
        raise ValueError("build_store: the dataset is empty")
    H, W = dataset.size
    store = np.empty((n, 3, H, W), dtype=np.uint8)
    targets = np.empty(n, dtype=np.int64)

    def one(i):
        a, targets[i] = dataset.load_u8(i)
        store[i] = a
        return bool((a[0] == a[1]).all() and (a[0] == a[2]).all())

    if workers == 1:
        gray = [one(i) for i in range(n)]
    else:
        with ThreadPoolExecutor(max_workers=workers) as pool:
            gray = list(pool.map(one, range(n)))
    return (np.ascontiguousarray(store[:, :1]) if all(gray) else store), targets


def store_manifest(dataset) -> dict:
    """What a cached store depends on, read from the directory as it is now: format version, preprocess, image size, Pillow's version and
    per sample (relative path, file size, mtime_ns, target).  The normalisation constants are not in it: the bytes do not depend on them."""
    import PIL
    samples = []
    for path, target in dataset.samples:
        st = os.stat(path)
        samples.append([os.path.relpath(path, dataset.root), st.st_size, st.st_mtime_ns, int(target)])
    return {"format": STORE_FORMAT, "preprocess": dataset.preprocess, "size": list(dataset.size), "pillow": PIL.__version__, "samples": samples}


def _read_store(cache_path: str, manifest: dict):
    """(store, targets) of a cache file whose manifest equals `manifest`, else None (also for a truncated or unreadable file)."""
    import json
    import numpy as np
    try:
        with np.load(cache_path, allow_pickle=False) as z:
            saved = json.loads(bytes(z["manifest"]).decode("utf-8"))
            channels = saved.pop("channels")
            if saved != manifest:
                return None
            store, targets = z["store"], z["targets"]
    except Exception:                                       # missing, truncated, not a zip, a missing member, not JSON: rebuild
        return None
    n = len(manifest["samples"])
    if store.dtype != np.uint8 or store.shape != (n, channels, *manifest["size"]) or channels not in (1, 3):
        return None
    if targets.dtype != np.int64 or targets.shape != (n,) or targets.tolist() != [s[3] for s in manifest["samples"]]:
        return None
    return store, targets


def load_or_build_store(dataset, cache_path: str, workers=None):
    """build_store through one uncompressed .npz (store, targets, manifest; read with allow_pickle=False): reused when its manifest equals
    store_manifest(dataset), otherwise rebuilt and replaced atomically (a temporary file in the same directory, then os.replace)."""
    import json
    import tempfile
    import numpy as np
    manifest = store_manifest(dataset)
    got = _read_store(cache_path, manifest)
    if got is not None:
        return got
    store, targets = build_store(dataset, workers)
    blob = json.dumps(dict(manifest, channels=int(store.shape[1]))).encode("utf-8")
    d = os.path.dirname(os.path.abspath(cache_path))
    os.makedirs(d, exist_ok=True)
    fd, tmp = tempfile.mkstemp(dir=d, prefix=os.path.basename(cache_path) + ".", suffix=".tmp")
    try:
        with os.fdopen(fd, "wb") as f:
            np.savez(f, store=store, targets=targets, manifest=np.frombuffer(blob, dtype=np.uint8))
        os.replace(tmp, cache_path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise
    return store, targets


def check_indices(idx, n: int) -> torch.Tensor:
    """The indices of one batch request as a CPU int64 tensor [B >= 1], every one in [0, n); anything else is refused here, on the host,
    before an index reaches the device."""
    idx = torch.as_tensor(idx)
    if idx.is_cuda:
        raise ValueError("batch indices must be on the CPU (they come from a CPU sampler and are range-checked before the upload)")
    if idx.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
        raise TypeError(f"batch indices must be integers (dtype={idx.dtype})")
    if idx.dim() != 1:
        raise ValueError(f"batch indices must be one-dimensional (shape={tuple(idx.shape)})")
    if idx.numel() < 1:
        raise ValueError("a batch needs at least one index")
    idx = idx.to(torch.int64).contiguous()
    lo, hi = int(idx.min()), int(idx.max())
    if lo < 0 or hi >= n:
        raise IndexError(f"batch indices must lie in [0, {n}) (min={lo}, max={hi})")
    return idx


def _free_device_bytes(device) -> int:
    return int(torch.cuda.mem_get_info(device)[0])


class IndexBatchLoader:
    """An iterable with __len__ over image_set.batch(idx): the index batches come from a real torch.utils.data.DataLoader over an
    index-only dataset with the same arguments, so the order -- and every draw from the generator (or the global one) -- is that of
    DataLoader(dataset, batch_size, shuffle, generator=generator, drop_last=drop_last), with no restatement of torch's samplers."""

    def __init__(self, image_set, batch_size: int, shuffle: bool = False, generator=None, drop_last: bool = False):
        self.image_set = image_set
        self.indices = torch.utils.data.DataLoader(range(len(image_set)), batch_size=batch_size, shuffle=shuffle, generator=generator,
                                                   drop_last=drop_last)

    def __len__(self):
        return len(self.indices)

    def __iter__(self):
        for idx in self.indices:
            yield self.image_set.batch(idx)


class DeviceImageSet:
    """An ImageFolderDataset decoded once and held on the GPU as bytes: store uint8 [N, Cs, H, W] (device), targets int64 [N] (CPU), lut
    float32 [3, 256] (device; dataset.byte_table()).  batch(idx) forms a batch with one nd_img_gather_u8 launch, bit for bit the tensors
    DataLoader(dataset) collates.  cache_path: the decoded store is kept in / reused from that file (load_or_build_store).  max_bytes
    (default: half of the free device memory now): a larger store is refused before anything is decoded."""

    def __init__(self, dataset, device="cuda", workers=None, cache_path=None, max_bytes=None):
        n, (H, W) = len(dataset), dataset.size
        if n < 1:
            raise ValueError("DeviceImageSet: the dataset is empty")
        self.device = torch.device(device)
        if max_bytes is None:
            max_bytes = _free_device_bytes(self.device) // 2
        self._refuse_above(n * (1 if dataset.preprocess == "grayscaled" else 3) * H * W, int(max_bytes))
        store, targets = load_or_build_store(dataset, cache_path, workers) if cache_path else build_store(dataset, workers)
        self._refuse_above(store.nbytes, int(max_bytes))
        self.size, self.targets = (H, W), torch.from_numpy(targets)
        self.store = torch.empty(store.shape, dtype=torch.uint8, device=self.device)
        rows = max(1, UPLOAD_CHUNK // max(1, store[0].nbytes))
        for lo in range(0, n, rows):
            self.store[lo:lo + rows].copy_(torch.from_numpy(store[lo:lo + rows]))
        self.lut = dataset.byte_table().to(self.device)

    @staticmethod
    def _refuse_above(need: int, max_bytes: int) -> None:
        if need > max_bytes:
            raise MemoryError(f"the decoded image store takes {need} bytes, above max_bytes={max_bytes}: train with the default loaders "
                              f"(cache 'none') or raise max_bytes")

    def __len__(self):
        return self.store.shape[0]

    def batch(self, idx):
        """(images float32 [B, 3, H, W] on the device, labels int64 [B] on the CPU) for CPU indices idx [B]."""
        from . import _lib
        idx = check_indices(idx, len(self))
        B, (H, W) = idx.numel(), self.size
        idx_dev = idx.to(torch.int32).to(self.device)
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=self.device)
        _lib.check(_lib.load().nd_img_gather_u8(_lib.ptr(self.store), len(self), self.store.shape[1], H * W, _lib.ptr(idx_dev), B,
                                                _lib.ptr(self.lut), _lib.ptr(out), _lib.current_stream_ptr(self.device)), "nd_img_gather_u8")
        return out, self.targets[idx]

    def loader(self, batch_size: int, shuffle: bool = False, generator=None, drop_last: bool = False) -> IndexBatchLoader:
        return IndexBatchLoader(self, batch_size, shuffle=shuffle, generator=generator, drop_last=drop_last)


def split_loader(root: str, split: str, dataset: str, preprocess: str, image_size, batch_size: int, cache: str = "none",
                 flag: str = "cache", cache_dir=None, device=None, workers=None, num_workers: int = 0, **order):
    """The training-time loader of <root>/<split>: a DataLoader over the ImageFolderDataset (num_workers processes), or with cache
    'device' the same batches in the same order from a DeviceImageSet on `device` (default 'cuda'; decoded by `workers` threads, kept
    in cache_file(cache_dir, split, ...)).  **order: shuffle, generator and drop_last, for either.  `flag` is the name the caller's
    setting goes by in the refusal of a cache outside CACHE_CHOICES."""
    if cache not in CACHE_CHOICES:
        raise ValueError(f"{flag} must be one of {CACHE_CHOICES} ({flag}={cache!r})")
    ds = ImageFolderDataset(os.path.join(root, split), dataset, preprocess, image_size)
    if cache == "device":
        return DeviceImageSet(ds, device or "cuda", workers=workers, cache_path=cache_file(cache_dir, split, ds)).loader(batch_size, **order)
    return torch.utils.data.DataLoader(ds, batch_size=batch_size, num_workers=num_workers, **order)


ATTACKS = ("FGSM", "PGD", "BIM", "AUTOPGD", "CW")
ATTACKED_DATASETS = tuple(f"{d}Atk{a}" for d in ("ChestXRay", "ISICSkinCancer") for a in ATTACKS)   # diffusion/utils.py:165-177


def get_dataset(args, config):
    """The ChestXRay / ISICSkinCancer (+ *Validate, *Atk*) branches of diffusion/utils.py:146-177: returns the split the
    test / calibration loop iterates (testing, or validation for the *Validate names; for the attacked names the
    <dataroot>/Test_attacks_<NAME> tree that make_attacks writes, read as data_loader_attacks reads it)."""
    name = config.data.dataset
    if name in ATTACKED_DATASETS:
        attack = name.split("Atk", 1)[1]
        return ImageFolderDataset(os.path.join(config.data.dataroot, f"Test_attacks_{attack}"), name.split("Atk", 1)[0], "attacked")
    base = {"ChestXRay": "ChestXRay", "ISICSkinCancer": "ISICSkinCancer", "ChestXRayValidate": "ChestXRay",
            "ISICSkinCancerValidate": "ISICSkinCancer"}.get(name)
    if base is None:
        raise NotImplementedError(f"dataset '{name}' is outside the accelerated path")
    split = "validation" if name.endswith("Validate") else "testing"
    return ImageFolderDataset(os.path.join(config.data.dataroot, split), base, args.preprocess)


def get_test_loader(args, config, shard=None):
    """The test loader of classification_train_separately.py:674-681 (batch_size from the config, no shuffle, drop_last).
    shard = (lo, hi): this rank's rows of every global batch -- the loader then yields [hi - lo] images and their targets per
    batch (attributes .shard / .global_batch say so), and only those files are opened."""
    n = int(getattr(args, "synthetic_batches", 0) or 0)
    B = config.testing.batch_size
    if n > 0:
        size = int(round((config.model.data_dim / 3) ** 0.5))          # 224 for data_dim = 150528 (3 x 224 x 224)
        if 3 * size * size != config.model.data_dim:
            raise ValueError(f"model.data_dim={config.model.data_dim} is not 3 x S x S")
        return SyntheticLoader(n, B, config.data.num_classes, seed=getattr(args, "seed", 0) or 0, size=size, shard=shard)
    ds = get_dataset(args, config)
    lo, hi = shard if shard is not None else (0, B)
    # pinned batches: the runner uploads them with a non-blocking copy on a side stream (upload.rank_batches) without a staging copy
    loader = torch.utils.data.DataLoader(ds, batch_sampler=ShardBatchSampler(len(ds), B, lo, hi),
                                         num_workers=int(getattr(config.data, "num_workers", 0) or 0), pin_memory=torch.cuda.is_available())
    loader.shard = (lo, hi) if shard is not None else None
    loader.global_batch = B
    return loader
