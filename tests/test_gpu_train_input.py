"""The training input on the GPU: nd_img_gather_u8 against lut[c][store[idx]] formed with torch (bit-equal: the kernel does no arithmetic on
values), its index guard and refusals, data.DeviceImageSet against the dataset it was built from, and the three trainers fed from the
device set against the same trainers fed by today's DataLoader (bit-identical checkpoints)."""
import argparse
import ctypes
import glob
import os

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import ref_cpu

pytestmark = pytest.mark.gpu
DEV = "cuda"


def gen(seed):
    return torch.Generator().manual_seed(seed)


def lib():
    from nested_diffusion_amd import _lib
    return _lib.load()


def stream():
    from nested_diffusion_amd import _lib
    return _lib.current_stream_ptr()


def bits(t):
    return t.contiguous().view(torch.int32)


def gather(store, n, cs, pixels, idx_dev, lut, out):
    from nested_diffusion_amd import _lib
    _lib.check(lib().nd_img_gather_u8(store.data_ptr(), n, cs, pixels, idx_dev.data_ptr(), idx_dev.numel(), lut.data_ptr(), out.data_ptr(),
                                      stream()), "nd_img_gather_u8")
    return out


def reference(store, cs, idx, lut):
    """lut[c][store[idx[b]][cs == 1 ? 0 : c][p]] with torch's indexing; store [n, cs, pixels] uint8, idx a list"""
    rows = store[torch.as_tensor(idx, device=store.device)].long()
    return torch.stack([lut[c][rows[:, 0 if cs == 1 else c]] for c in range(3)], dim=1)


def index_lists(B, n):
    """reversed order from the last row down, wrapping (so B > n repeats rows, and B >= n holds the first and the last row); for B = 1
    the first row as well"""
    lists = [[(n - 1 - i) % n for i in range(B)]]
    return lists + ([[0]] if B == 1 and n > 1 else [])


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pixels", [1, 3, 4, 5, 35, 1024])
def test_gather_equals_the_table_lookup_bit_for_bit(pixels):
    """pixels % 4 == 0 takes the four-byte form, everything else the scalar one; 1024 is more than one pass of a workgroup's lanes in the
    scalar form and exactly one in the vector form, 35 a row the lanes do not fill."""
    lut = torch.randn(3, 256, generator=gen(1)).to(DEV)
    for cs in (1, 3):
        for n in (1, 7):
            store = torch.randint(0, 256, (n, cs, pixels), dtype=torch.uint8, generator=gen(10 * n + cs)).to(DEV)
            for B in (1, 2, 31):
                for idx in index_lists(B, n):
                    out = torch.full((B, 3, pixels), float("nan"), device=DEV)
                    gather(store, n, cs, pixels, torch.tensor(idx, dtype=torch.int32, device=DEV), lut, out)
                    assert torch.equal(bits(out), bits(reference(store, cs, idx, lut))), (cs, n, B, idx)


@pytest.mark.parametrize("cs", [1, 3])
def test_gather_at_the_production_row(cs):
    """224 x 224 = 50176 pixels: 25 workgroups per row, the last one partly filled; a batch of 30 from 41 images"""
    pixels, n, B = 50176, 41, 30
    lut = torch.randn(3, 256, generator=gen(2)).to(DEV)
    store = torch.randint(0, 256, (n, cs, pixels), dtype=torch.uint8, generator=gen(3)).to(DEV)
    idx = torch.randperm(n, generator=gen(4))[:B].tolist()
    out = gather(store, n, cs, pixels, torch.tensor(idx, dtype=torch.int32, device=DEV), lut, torch.empty(B, 3, pixels, device=DEV))
    assert torch.equal(bits(out), bits(reference(store, cs, idx, lut)))


@pytest.mark.parametrize("shift_store,shift_out", [(1, 0), (2, 0), (0, 1), (3, 3), (4, 4)])
def test_a_misaligned_base_takes_the_scalar_form_with_the_same_results(shift_store, shift_out):
    """pixels % 4 == 0, but the store does not start on a 4-byte boundary or the output not on a 16-byte one: bytes and floats one by one.
    (4, 4): both aligned again, the store at 4 bytes and the output at 16."""
    pixels, n, cs, B = 1024, 3, 3, 5
    lut = torch.randn(3, 256, generator=gen(5)).to(DEV)
    flat = torch.randint(0, 256, (n * cs * pixels + 8,), dtype=torch.uint8, generator=gen(6)).to(DEV)
    store = flat[shift_store:shift_store + n * cs * pixels].view(n, cs, pixels)
    outbuf = torch.full((B * 3 * pixels + 8,), float("nan"), device=DEV)
    out = outbuf[shift_out:shift_out + B * 3 * pixels].view(B, 3, pixels)
    assert store.data_ptr() % 4 == shift_store % 4 and out.data_ptr() % 16 == 4 * shift_out % 16
    idx = [2, 0, 1, 1, 2]
    gather(store, n, cs, pixels, torch.tensor(idx, dtype=torch.int32, device=DEV), lut, out)
    assert torch.equal(bits(out), bits(reference(store, cs, idx, lut)))
    rest = torch.cat([outbuf[:shift_out], outbuf[shift_out + B * 3 * pixels:]])
    assert bool(rest.isnan().all())                                           # nothing written outside the batch


def test_offsets_into_the_store_are_64_bit():
    """28600 rows of 150528 bytes (3 x 224 x 224): 4.31 GB, the last row starts above 2^32.  The store is allocated uninitialised and only
    rows 0 and N - 1 are written and gathered."""
    n, cs, pixels = 28600, 3, 50176
    assert (n - 1) * cs * pixels > 2 ** 32
    store = torch.empty((n, cs, pixels), dtype=torch.uint8, device=DEV)
    ends = torch.randint(0, 256, (2, cs, pixels), dtype=torch.uint8, generator=gen(7)).to(DEV)
    store[0].copy_(ends[0])
    store[n - 1].copy_(ends[1])
    lut = torch.randn(3, 256, generator=gen(8)).to(DEV)
    out = gather(store, n, cs, pixels, torch.tensor([n - 1, 0], dtype=torch.int32, device=DEV), lut, torch.empty(2, 3, pixels, device=DEV))
    assert torch.equal(bits(out), bits(reference(ends, cs, [1, 0], lut)))
    del store


@pytest.mark.parametrize("cs,pixels", [(1, 35), (3, 1024)])
def test_rows_with_an_index_outside_the_store_are_left_alone(cs, pixels):
    """Indices -1 and n_images (raw ctypes: the Python wrapper refuses them on the host) read nothing and write nothing; the rows beside
    them are right.  The store handed over is rows 1 .. N of an allocation of N + 2 rows, so every address the indices could name lies
    inside memory this test owns."""
    n, sentinel = 5, -7.25
    whole = torch.randint(0, 256, (n + 2, cs, pixels), dtype=torch.uint8, generator=gen(9)).to(DEV)
    store = whole[1:n + 1]
    lut = torch.randn(3, 256, generator=gen(10)).to(DEV)
    idx = [-1, 0, n, n - 1, 2, -1]
    out = torch.full((len(idx), 3, pixels), sentinel, device=DEV)
    rc = lib().nd_img_gather_u8(store.data_ptr(), n, cs, pixels, torch.tensor(idx, dtype=torch.int32, device=DEV).data_ptr(), len(idx),
                                lut.data_ptr(), out.data_ptr(), stream())
    assert rc == 0
    good = [b for b, i in enumerate(idx) if 0 <= i < n]
    assert good == [1, 3, 4]
    assert torch.equal(bits(out[good]), bits(reference(store, cs, [idx[b] for b in good], lut)))
    for b in (0, 2, 5):
        assert bool((out[b] == sentinel).all()), b


def test_every_refusal_of_the_entry_point():
    L = lib()
    buf = torch.zeros(64, device=DEV)
    P = buf.data_ptr()                                       # a real, 16-byte aligned device address; nothing is launched
    cases = [
        (lambda: L.nd_img_gather_u8(None, 1, 1, 4, P, 1, P, P, None), b"NULL"),
        (lambda: L.nd_img_gather_u8(P, 1, 1, 4, None, 1, P, P, None), b"NULL"),
        (lambda: L.nd_img_gather_u8(P, 1, 1, 4, P, 1, None, P, None), b"NULL"),
        (lambda: L.nd_img_gather_u8(P, 1, 1, 4, P, 1, P, None, None), b"NULL"),
        (lambda: L.nd_img_gather_u8(P, 1, 0, 4, P, 1, P, P, None), b"src_channels=0"),
        (lambda: L.nd_img_gather_u8(P, 1, 2, 4, P, 1, P, P, None), b"src_channels=2"),
        (lambda: L.nd_img_gather_u8(P, 1, 4, 4, P, 1, P, P, None), b"src_channels=4"),
        (lambda: L.nd_img_gather_u8(P, 1, 1, 0, P, 1, P, P, None), b"pixels=0"),
        (lambda: L.nd_img_gather_u8(P, 1, 1, -4, P, 1, P, P, None), b"pixels=-4"),
        (lambda: L.nd_img_gather_u8(P, 1, 1, 4, P, 0, P, P, None), b"B=0"),
        (lambda: L.nd_img_gather_u8(P, 0, 1, 4, P, 1, P, P, None), b"n_images=0"),
        (lambda: L.nd_img_gather_u8(P, -3, 1, 4, P, 1, P, P, None), b"n_images=-3"),
        (lambda: L.nd_img_gather_u8(P, 1, 1, 4, P + 2, 1, P, P, None), b"aligned"),
        (lambda: L.nd_img_gather_u8(P, 1, 1, 4, P, 1, P + 1, P, None), b"aligned"),
        (lambda: L.nd_img_gather_u8(P, 1, 1, 4, P, 1, P, P + 3, None), b"aligned"),
    ]
    for i, (call, words) in enumerate(cases):
        assert call() != 0, i
        assert words in L.nd_last_error(), (i, L.nd_last_error())
    torch.cuda.synchronize()
    assert bool((buf == 0).all())


# ---- 2. DeviceImageSet ---------------------------------------------------------------------------------------------------------------
def image_tree(root, seed=0):
    """two class folders of PNG and JPEG files at 37 x 53, 300 x 200, 224 x 224 and 16 x 16 (width x height)"""
    rng = np.random.RandomState(seed)
    k = 0
    for c in ("NORMAL", "PNEUMONIA"):
        os.makedirs(os.path.join(root, c))
        for (w, h) in ((37, 53), (300, 200), (224, 224), (16, 16)):
            a = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
            a[:, : w // 2] = a[:, : w // 2] // 4 + 100 * (k % 2)          # structure a JPEG keeps
            Image.fromarray(a, "RGB").save(os.path.join(root, c, f"{k}.{'png' if k % 2 == 0 else 'jpg'}"), **({} if k % 2 == 0 else {"quality": 90}))
            k += 1
    return root


@pytest.fixture(scope="module")
def tree_root(tmp_path_factory):
    return image_tree(str(tmp_path_factory.mktemp("images")))


@pytest.mark.parametrize("preprocess,size", [("grayscaled", (32, 32)), ("standardized", (32, 32)), ("attacked", (32, 32)),
                                             ("grayscaled", (224, 224)), ("standardized", (40, 24))])
def test_device_set_returns_the_datasets_tensors(tree_root, preprocess, size):
    from nested_diffusion_amd.data import DeviceImageSet, ImageFolderDataset
    ds = ImageFolderDataset(tree_root, "ISICSkinCancer", preprocess, image_size=size)
    dev = DeviceImageSet(ds, DEV, workers=3)
    assert len(dev) == len(ds) == 8 and dev.store.dtype == torch.uint8 and dev.store.is_cuda and dev.lut.is_cuda and not dev.targets.is_cuda
    assert tuple(dev.store.shape) == (8, 1 if preprocess == "grayscaled" else 3, *size)
    for i in range(len(ds)):
        x, t = ds[i]
        got, labels = dev.batch([i])
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (1, 3, *size)
        assert not labels.is_cuda and labels.dtype == torch.int64 and labels.tolist() == [t]
        assert torch.equal(bits(got[0].cpu()), bits(x)), i
    for bad in ([8], [-1], [], [0.5]):
        with pytest.raises((IndexError, ValueError, TypeError)):
            dev.batch(bad)


def test_device_set_loader_yields_the_dataloaders_batches(tree_root, tmp_path):
    from nested_diffusion_amd.data import DeviceImageSet, ImageFolderDataset
    ds = ImageFolderDataset(tree_root, "ChestXRay", "standardized", image_size=(32, 32))
    cache = str(tmp_path / "set.npz")
    dev = DeviceImageSet(ds, DEV, cache_path=cache)
    again = DeviceImageSet(ds, DEV, cache_path=cache)                       # from the file
    assert os.path.exists(cache) and torch.equal(dev.store, again.store) and torch.equal(dev.targets, again.targets)
    ref = torch.utils.data.DataLoader(ds, batch_size=3, shuffle=True, generator=gen(21))
    mine = again.loader(3, shuffle=True, generator=gen(21))
    assert len(mine) == len(ref) == 3
    orders = []
    for _ in range(2):
        a, b = list(ref), list(mine)
        assert len(a) == len(b) == 3 and [x.shape[0] for x, _ in b] == [3, 3, 2]
        for (xa, ta), (xb, tb) in zip(a, b):
            assert xb.is_cuda and not tb.is_cuda and torch.equal(ta, tb) and ta.dtype == tb.dtype
            assert torch.equal(bits(xa), bits(xb.cpu()))
        orders.append(torch.cat([t for _, t in b]).tolist())
    assert len(list(again.loader(3, drop_last=True))) == 2


def test_a_store_above_max_bytes_is_refused_with_both_numbers(tree_root):
    from nested_diffusion_amd.data import DeviceImageSet, ImageFolderDataset
    ds = ImageFolderDataset(tree_root, "ChestXRay", "grayscaled", image_size=(32, 32))
    with pytest.raises(MemoryError, match="8192 bytes.*max_bytes=8191"):
        DeviceImageSet(ds, DEV, max_bytes=8191)
    assert len(DeviceImageSet(ds, DEV, max_bytes=8192)) == 8


# ---- 3. the trainers reach the same weights ------------------------------------------------------------------------------------------
IMG, PATCH, EMBED = 32, 16, 128


@pytest.fixture(scope="module")
def split_root(tmp_path_factory):
    """<root>/{training,validation}/<class>/: 10 + 6 small files, PNG and JPEG, class-dependent brightness"""
    root = str(tmp_path_factory.mktemp("splits"))
    rng = np.random.RandomState(12)
    for split, n in (("training", 5), ("validation", 3)):
        for ci, c in enumerate(("NORMAL", "PNEUMONIA")):
            os.makedirs(os.path.join(root, split, c))
            for i in range(n):
                a = (rng.randint(0, 120, (40 + i, 36, 3)) + 110 * ci).astype(np.uint8)
                Image.fromarray(a, "RGB").save(os.path.join(root, split, c, f"{i}.{'png' if i % 2 else 'jpg'}"))
    return root


def same_state(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) and (not a[k].is_floating_point() or torch.equal(bits(a[k]), bits(b[k]))), k


def loaders(root, cache, tmp_path, batch=4, seed=3):
    from nested_diffusion_amd import train_mapping as tm
    return tm.make_loaders(root, "ChestXRay", "grayscaled", batch, seed, cache=cache, cache_dir=str(tmp_path / "cache"), workers=2, device=DEV,
                           image_size=(IMG, IMG))


def test_mapping_trainer_reaches_the_same_weights_from_the_device_set(split_root, tmp_path, capsys):
    from nested_diffusion_amd.data import IndexBatchLoader
    from nested_diffusion_amd.mapping import VisionTransformer
    from nested_diffusion_amd.train_mapping import MappingTrainer
    vit = VisionTransformer(ref_cpu.init_vit_params(embed=EMBED, depth=2, patch=PATCH, img=IMG, num_classes=2, seed=3), 2, DEV)
    res = {}
    for cache in ("none", "device"):
        train, valid = loaders(split_root, cache, tmp_path)
        assert isinstance(train, IndexBatchLoader if cache == "device" else torch.utils.data.DataLoader) and len(train) == 3 and len(valid) == 1
        tr = MappingTrainer(vit, 1, num_classes=2, lr=1e-3, seed=0, in_features=(IMG // PATCH) ** 2 * EMBED, hidden=(32, 16, 16))
        hist = tr.fit(train, valid, 2, str(tmp_path / cache))
        assert tr.t == 6 and hist["saved_epochs"]
        res[cache] = (hist, torch.load(hist["path"]), tr.state_dict())
    capsys.readouterr()
    assert sorted(os.listdir(str(tmp_path / "cache"))) == [f"training_grayscaled_{IMG}x{IMG}.npz", f"validation_grayscaled_{IMG}x{IMG}.npz"]
    (ha, fa, sa), (hb, fb, sb) = res["none"], res["device"]
    assert {k: v for k, v in ha.items() if k != "path"} == {k: v for k, v in hb.items() if k != "path"}
    same_state(fa, fb)
    same_state(sa, sb)


def test_vit_trainer_reaches_the_same_weights_from_the_device_set(split_root, tmp_path, capsys):
    from nested_diffusion_amd import train_transformer as tt
    init = tt.init_state_dict(num_classes=2, embed=EMBED, depth=1, patch=PATCH, img=IMG, seed=2)
    res = {}
    for cache in ("none", "device"):
        train, valid = loaders(split_root, cache, tmp_path)
        tr = tt.ViTTrainer(init, num_classes=2, num_heads=2)
        hist = tr.fit(train, valid, 1, str(tmp_path / cache), "ChestXRay")
        assert tr.t == 3 and hist["saved_epochs"] == [0]
        res[cache] = (hist, torch.load(hist["path"]), tr.state_dict())
    capsys.readouterr()
    (ha, fa, sa), (hb, fb, sb) = res["none"], res["device"]
    assert {k: v for k, v in ha.items() if k != "path"} == {k: v for k, v in hb.items() if k != "path"}
    same_state(fa, fb)
    same_state(sa, sb)


def test_diffusion_train_writes_the_same_checkpoint_with_the_device_set(split_root, tmp_path):
    from nested_diffusion_amd.mapping import Classifier, GuidingConditioner, VisionTransformer
    from nested_diffusion_amd.runner import Diffusion
    ns = argparse.Namespace
    depth, K, B, C, T = 2, 2, 4, 2, 5
    vp = ref_cpu.init_vit_params(embed=EMBED, depth=depth, patch=PATCH, img=IMG, seed=5)
    mlps = [ref_cpu.init_classifier_params((IMG // PATCH) ** 2 * EMBED, widths=(64, 32, 16), seed=10 + i) for i in range(K)]
    cond = GuidingConditioner(VisionTransformer(vp, 2), [Classifier(m) for m in mlps])
    files = {}
    for cache in ("none", "device"):
        cfg = ns(data=ns(dataset="ChestXRay", dataroot=split_root, num_classes=C, num_workers=0, label_min_max=[0.001, 0.999]),
                 model=ns(data_dim=3 * IMG * IMG, hidden_dim=32, feature_dim=32, arch="linear"),
                 diffusion=ns(timesteps=T, beta_schedule="linear", beta_start=1e-4, beta_end=0.02, aux_cls=ns(arch="sevit"), include_guidance=True,
                              trained_aux_cls_ckpt_path="", trained_diffusion_ckpt_path=[[]]),
                 optim=ns(optimizer="Adam", lr=1e-3, beta1=0.9, eps=1e-8, weight_decay=0.0, amsgrad=False, grad_clip=1.0, lr_schedule=True, min_lr=0.0),
                 training=ns(batch_size=B, n_epochs=2, warmup_epochs=1, validation_freq=1, logging_freq=0), testing=ns(batch_size=3))
        out = tmp_path / cache
        out.mkdir()
        args = ns(seed=7, mc_trials=2, log_path=str(out), preprocess="grayscaled", train_cache=cache, cache_dir=None)
        torch.manual_seed(7)                                  # the shuffle, the timesteps and e are drawn from the global generators
        res = Diffusion(args, cfg, device=DEV, conditioner=cond).train(1)
        assert len(res["losses"]) == 2 and res["best"]
        files[cache] = (res, sorted(os.path.basename(f) for f in glob.glob(str(out / "*.pth"))), torch.get_rng_state())
    (ra, na, ga), (rb, nb, gb) = files["none"], files["device"]
    assert na == nb and ra["losses"] == rb["losses"] and ra["accuracies"] == rb["accuracies"] and torch.equal(ga, gb)
    a, b = torch.load(ra["best"]), torch.load(rb["best"])
    assert a["epoch"] == b["epoch"] and a["optimizer"] == b["optimizer"]
    same_state(a["noise_estimator"], b["noise_estimator"])
