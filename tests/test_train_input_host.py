"""The training input's host side (data.py): the byte -> float table against __getitem__, build_store / load_or_build_store, the batch
request's refusals, the memory refusal, the index loader's order against torch's DataLoader, and the three command lines' new flags.
No GPU and no library: everything here is a pure host function."""
import os

import numpy as np
import pytest
import torch

from PIL import Image

from nested_diffusion_amd import data


def all_bytes_image(path, grey):
    """16 x 16 RGB holding all 256 byte values in every channel: each channel in another order, or (grey) three equal planes, which the
    L conversion returns as they are"""
    v = np.arange(256, dtype=np.uint8)
    a = np.stack([v, v, v] if grey else [v, v[::-1], np.roll(v, 77)], axis=-1).reshape(16, 16, 3)
    Image.fromarray(a, "RGB").save(path)
    return a


def tree(root, n_per_class=3, size=(20, 24), seed=0, colour=True):
    """<root>/{a,b}/<i>.png of random pixels; returns the root"""
    rng = np.random.RandomState(seed)
    for c in ("a", "b"):
        os.makedirs(os.path.join(root, c), exist_ok=True)
        for i in range(n_per_class):
            a = rng.randint(0, 256, (*size, 3)).astype(np.uint8)
            Image.fromarray(a if colour else a[:, :, :1].repeat(3, 2), "RGB").save(os.path.join(root, c, f"{i}.png"))
    return root


# ---- 1. the byte transform -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,preprocess", [("ChestXRay", "grayscaled"), ("ChestXRay", "standardized"), ("ISICSkinCancer", "standardized"),
                                             ("ChestXRay", "attacked")])
def test_byte_table_of_load_u8_is_getitem_bit_for_bit(tmp_path, name, preprocess):
    os.makedirs(tmp_path / "c")
    a = all_bytes_image(str(tmp_path / "c" / "all.png"), grey=preprocess == "grayscaled")
    ds = data.ImageFolderDataset(str(tmp_path), name, preprocess, image_size=(16, 16))
    u8, target = ds.load_u8(0)
    x, target2 = ds[0]
    assert u8.dtype == np.uint8 and u8.shape == (3, 16, 16) and target == target2 == 0
    assert np.array_equal(u8, a.transpose(2, 0, 1))                      # a same-size resize is the identity
    lut = ds.byte_table()
    assert lut.dtype == torch.float32 and tuple(lut.shape) == (3, 256) and lut.is_contiguous()
    for c in range(3):
        assert len(np.unique(u8[c])) == 256
        got = lut[c][torch.from_numpy(u8[c]).long()]
        assert got.dtype == x.dtype and torch.equal(got.view(torch.int32), x[c].view(torch.int32)), c
    if preprocess == "standardized":
        assert not torch.equal(lut[0], lut[1])
    else:
        assert torch.equal(lut[0], torch.arange(256).float() / 255) and torch.equal(lut[0], lut[2])


# ---- 2. build_store ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("workers", [1, 3])
@pytest.mark.parametrize("preprocess,cs", [("grayscaled", 1), ("standardized", 3)])
def test_build_store_equals_load_u8(tmp_path, workers, preprocess, cs):
    ds = data.ImageFolderDataset(tree(str(tmp_path)), "ChestXRay", preprocess, image_size=(8, 12))
    store, targets = data.build_store(ds, workers=workers)
    assert store.dtype == np.uint8 and store.shape == (6, cs, 8, 12) and store.flags["C_CONTIGUOUS"]
    assert targets.dtype == np.int64 and targets.tolist() == [0, 0, 0, 1, 1, 1]
    for i in range(len(ds)):
        u8, t = ds.load_u8(i)
        assert np.array_equal(store[i], u8[:cs]) and t == targets[i]
        assert cs == 3 or (np.array_equal(u8[0], u8[1]) and np.array_equal(u8[0], u8[2]))


def test_build_store_keeps_one_plane_of_a_grey_tree_and_three_if_one_image_is_coloured(tmp_path):
    root = tree(str(tmp_path), colour=False)
    ds = data.ImageFolderDataset(root, "ChestXRay", "standardized", image_size=(8, 8))
    assert data.build_store(ds, workers=2)[0].shape[1] == 1
    Image.fromarray(np.random.RandomState(3).randint(0, 256, (9, 9, 3)).astype(np.uint8), "RGB").save(os.path.join(root, "b", "z.png"))
    ds = data.ImageFolderDataset(root, "ChestXRay", "standardized", image_size=(8, 8))
    assert data.build_store(ds, workers=2)[0].shape == (7, 3, 8, 8)


def test_build_store_refuses_more_than_16_workers_and_an_empty_set(tmp_path):
    ds = data.ImageFolderDataset(tree(str(tmp_path)), "ChestXRay", "grayscaled", image_size=(8, 8))
    for bad in (17, 64, 0, -1):
        with pytest.raises(ValueError, match="workers"):
            data.build_store(ds, workers=bad)
    assert data._workers(None) == min(16, len(os.sched_getaffinity(0))) and data._workers(16) == 16
    ds.samples = []
    with pytest.raises(ValueError, match="empty"):
        data.build_store(ds, workers=1)


# ---- 3. load_or_build_store ----------------------------------------------------------------------------------------------------------
class Counting(data.ImageFolderDataset):
    calls = 0

    def load_u8(self, i):
        Counting.calls += 1
        return super().load_u8(i)


def counted(root, preprocess="grayscaled", size=(8, 8), cache=None):
    """(store, targets, number of load_u8 calls) of one load_or_build_store over the tree as it is now"""
    ds = Counting(root, "ChestXRay", preprocess, image_size=size)
    Counting.calls = 0
    store, targets = data.load_or_build_store(ds, cache, workers=2)
    ref = data.build_store(data.ImageFolderDataset(root, "ChestXRay", preprocess, image_size=size), workers=1)
    assert np.array_equal(store, ref[0]) and np.array_equal(targets, ref[1]) and store.dtype == np.uint8 and targets.dtype == np.int64
    return store, targets, Counting.calls


def test_cache_file_is_reused_and_every_change_rebuilds_it(tmp_path):
    root, cache = tree(str(tmp_path / "data")), str(tmp_path / "cache" / "train.npz")
    assert counted(root, cache=cache)[2] == 6 and os.path.exists(cache)
    assert os.listdir(os.path.dirname(cache)) == ["train.npz"]              # the temporary file is gone
    with np.load(cache, allow_pickle=False) as z:
        assert sorted(z.files) == ["manifest", "store", "targets"]
    assert counted(root, cache=cache)[2] == 0                                # a second call decodes nothing
    # a touched file
    st = os.stat(os.path.join(root, "a", "1.png"))
    os.utime(os.path.join(root, "a", "1.png"), ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))
    assert counted(root, cache=cache)[2] == 6 and counted(root, cache=cache)[2] == 0
    # an added file
    Image.fromarray(np.full((5, 5, 3), 9, np.uint8), "RGB").save(os.path.join(root, "b", "added.png"))
    assert counted(root, cache=cache)[2] == 7 and counted(root, cache=cache)[2] == 0
    # another preprocess, another size
    assert counted(root, preprocess="standardized", cache=cache)[2] == 7 and counted(root, preprocess="standardized", cache=cache)[2] == 0
    assert counted(root, preprocess="standardized", size=(8, 9), cache=cache)[2] == 7
    assert counted(root, preprocess="standardized", size=(8, 9), cache=cache)[2] == 0
    # a truncated file, an empty file, a file that is no archive
    blob = open(cache, "rb").read()
    for broken in (blob[:len(blob) // 2], b"", b"not an archive"):
        with open(cache, "wb") as f:
            f.write(broken)
        assert counted(root, preprocess="standardized", size=(8, 9), cache=cache)[2] == 7
        assert counted(root, preprocess="standardized", size=(8, 9), cache=cache)[2] == 0
    assert os.listdir(os.path.dirname(cache)) == ["train.npz"]


def test_manifest_names_what_the_store_depends_on(tmp_path):
    import PIL
    root = tree(str(tmp_path))
    m = data.store_manifest(data.ImageFolderDataset(root, "ChestXRay", "grayscaled", image_size=(8, 12)))
    assert m["format"] == data.STORE_FORMAT and m["preprocess"] == "grayscaled" and m["size"] == [8, 12] and m["pillow"] == PIL.__version__
    assert [s[0] for s in m["samples"]] == [os.path.join(c, f"{i}.png") for c in "ab" for i in range(3)]
    assert all(s[1] == os.path.getsize(os.path.join(root, s[0])) and s[2] == os.stat(os.path.join(root, s[0])).st_mtime_ns for s in m["samples"])
    assert [s[3] for s in m["samples"]] == [0, 0, 0, 1, 1, 1]


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------
def test_check_indices():
    got = data.check_indices([3, 0, 3, 6], 7)
    assert got.dtype == torch.int64 and got.tolist() == [3, 0, 3, 6] and not got.is_cuda
    assert data.check_indices(torch.tensor([2], dtype=torch.int32), 3).dtype == torch.int64
    assert data.check_indices(np.array([0, 1]), 2).tolist() == [0, 1]
    for bad, exc in (([0.0, 1.0], TypeError), ([True, False], TypeError), ([[0, 1]], ValueError), (3, ValueError), ([], (ValueError, TypeError)),
                     (torch.zeros(0, dtype=torch.int64), ValueError), ([0, 7], IndexError), ([-1, 2], IndexError), ([2 ** 40], IndexError)):
        with pytest.raises(exc):
            data.check_indices(bad, 7)


def test_a_store_above_max_bytes_is_refused_before_anything_is_decoded(tmp_path, monkeypatch):
    root = tree(str(tmp_path))
    Counting.calls = 0
    with pytest.raises(MemoryError, match=r"384 bytes.*max_bytes=383"):                 # 6 images x 1 plane x 8 x 8
        data.DeviceImageSet(Counting(root, "ChestXRay", "grayscaled", image_size=(8, 8)), "cuda", max_bytes=383)
    with pytest.raises(MemoryError, match=r"1152 bytes.*max_bytes=1151"):               # three planes unless grayscaled
        data.DeviceImageSet(Counting(root, "ChestXRay", "standardized", image_size=(8, 8)), "cuda", max_bytes=1151)
    monkeypatch.setattr(data, "_free_device_bytes", lambda device: 700)                 # the default: half of the free memory
    with pytest.raises(MemoryError, match=r"384 bytes.*max_bytes=350"):
        data.DeviceImageSet(Counting(root, "ChestXRay", "grayscaled", image_size=(8, 8)), "cuda")
    assert Counting.calls == 0


# ---- 5. the index loader's order -----------------------------------------------------------------------------------------------------
class Echo:
    """a stand-in set: batch(idx) returns its indices"""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def batch(self, idx):
        return idx.clone()


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("n,batch", [(23, 5), (20, 5), (3, 7)])
def test_index_loader_order_is_the_dataloaders(shuffle, drop_last, n, batch):
    ref = torch.utils.data.DataLoader(torch.arange(n), batch_size=batch, shuffle=shuffle, drop_last=drop_last,
                                      generator=torch.Generator().manual_seed(5))
    mine = data.IndexBatchLoader(Echo(n), batch, shuffle=shuffle, drop_last=drop_last, generator=torch.Generator().manual_seed(5))
    assert len(mine) == len(ref) == (n // batch if drop_last else -(-n // batch))
    seen = []
    for _ in range(3):
        a, b = list(ref), list(mine)
        assert len(a) == len(b) == len(ref) and all(torch.equal(x, y) and y.dtype == torch.int64 for x, y in zip(a, b))
        seen.append(torch.cat(b).tolist() if b else [])
    if shuffle and n > batch:
        assert seen[0] != seen[1] and seen[0] != sorted(seen[0])             # a fresh permutation every epoch
    if not drop_last:
        assert sorted(seen[0]) == list(range(n))


def test_index_loader_draws_from_the_global_generator_as_the_dataloader_does():
    torch.manual_seed(11)
    a = [list(torch.utils.data.DataLoader(torch.arange(13), batch_size=4, shuffle=True)) for _ in range(2)]
    state_a = torch.get_rng_state()
    torch.manual_seed(11)
    mine = data.IndexBatchLoader(Echo(13), 4, shuffle=True)
    b = [list(mine) for _ in range(2)]
    assert torch.equal(torch.get_rng_state(), state_a)
    assert all(torch.equal(x, y) for ea, eb in zip(a, b) for x, y in zip(ea, eb))


# ---- 6. the command lines ------------------------------------------------------------------------------------------------------------
def test_parsers_default_to_no_cache_and_take_the_new_flags(capsys):
    from nested_diffusion_amd import main, train_mapping, train_transformer
    tm = ["--dataset", "ChestXRay", "--root_dir", "r", "--mn_idx", "0", "--vit", "v", "--out", "o"]
    tt = ["--dataset", "ChestXRay", "--root_dir", "r", "--out", "o"]
    for parser, base in ((train_mapping.build_parser(), tm), (train_transformer.build_parser(), tt)):
        assert train_mapping.cache_settings(parser.parse_args(base)) == dict(cache="none", cache_dir=None, workers=None)
        a = parser.parse_args(base + ["--cache", "device", "--cache_dir", "d", "--workers", "8"])
        assert train_mapping.cache_settings(a) == dict(cache="device", cache_dir="d", workers=8)
        assert train_mapping.cache_settings(parser.parse_args(base + ["--cache", "none"]))["cache"] == "none"
        with pytest.raises(SystemExit):
            parser.parse_args(base + ["--cache", "host"])
    mp, mb = main.build_parser(), ["--preprocess", "grayscaled", "--config", "c", "--doc", "d"]
    a = mp.parse_args(mb)
    assert (a.train_cache, a.cache_dir) == ("none", None)
    a = mp.parse_args(mb + ["--train_cache", "device", "--cache_dir", "d"])
    assert (a.train_cache, a.cache_dir) == ("device", "d")
    with pytest.raises(SystemExit):
        mp.parse_args(mb + ["--train_cache", "host"])
    capsys.readouterr()


def test_make_loaders_without_a_cache_is_the_dataloader_and_names_its_cache_files(tmp_path):
    from nested_diffusion_amd import train_mapping as tm
    for split in ("training", "validation"):
        tree(str(tmp_path / split))
    train, valid = tm.make_loaders(str(tmp_path), "ChestXRay", "grayscaled", 4, 3)
    assert isinstance(train, torch.utils.data.DataLoader) and isinstance(valid, torch.utils.data.DataLoader)
    assert train.dataset.size == (224, 224) and valid.batch_size == tm.VALID_BATCH
    assert tm.cache_file(None, "training", train.dataset) is None
    assert tm.cache_file("d", "training", train.dataset) == os.path.join("d", "training_grayscaled_224x224.npz")
    with pytest.raises(ValueError, match="cache"):
        tm.make_loaders(str(tmp_path), "ChestXRay", "grayscaled", 4, 3, cache="host")


def test_split_loader_builds_both_training_paths_loaders_from_their_arguments(tmp_path):
    """data.split_loader is the one place that turns a split into a loader: through train_mapping.make_loaders' arguments a shuffled
    DataLoader on the seeded generator, nothing dropped; through the noise-estimator loop's (train_diffusion.default_loader) num_workers
    from the config and drop_last on validation.  Each refusal names its own flag."""
    import argparse
    from nested_diffusion_amd import _trainer, train_diffusion as td, train_mapping as tm, train_transformer as tt
    assert tm.make_loaders is tt.make_loaders is _trainer.make_loaders and tm.snapshot_settings is _trainer.snapshot_settings
    ns = argparse.Namespace
    tree(str(tmp_path / "training"))                                                # 6 images
    tree(str(tmp_path / "validation"), n_per_class=4)
    os.remove(str(tmp_path / "validation" / "b" / "3.png"))                          # 7 images
    train, valid = tm.make_loaders(str(tmp_path), "ChestXRay", "grayscaled", 4, 3, image_size=(8, 8))
    assert isinstance(train, torch.utils.data.DataLoader) and isinstance(train.sampler, torch.utils.data.RandomSampler)
    assert isinstance(train.generator, torch.Generator) and train.generator.initial_seed() == 3 and train.num_workers == 0
    assert not train.drop_last and not valid.drop_last and isinstance(valid.sampler, torch.utils.data.SequentialSampler)
    assert valid.generator is None and len(train) == 2 and len(valid) == 1 and valid.batch_size == tm.VALID_BATCH
    ref = torch.utils.data.DataLoader(train.dataset, batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(3))
    assert all(torch.equal(a[1], b[1]) and torch.equal(a[0], b[0]) for a, b in zip(train, ref))
    # the noise-estimator loop's arguments
    cfg = ns(data=ns(dataroot=str(tmp_path), dataset="ChestXRay", num_workers=2), model=ns(data_dim=3 * 8 * 8))
    args = ns(preprocess="grayscaled")
    train = td.default_loader(args, cfg, "cuda", "training", 4, shuffle=True)
    valid = td.default_loader(args, cfg, "cuda", "validation", 3, shuffle=False, drop_last=True)
    assert isinstance(train, torch.utils.data.DataLoader) and train.num_workers == valid.num_workers == 2 and train.generator is None
    assert isinstance(train.sampler, torch.utils.data.RandomSampler) and train.dataset.size == (8, 8) and not train.drop_last
    assert valid.drop_last and len(valid.dataset) == 7 and len(valid) == 2 and isinstance(valid.sampler, torch.utils.data.SequentialSampler)
    # both refusals, word for word
    with pytest.raises(ValueError) as e:
        tm.make_loaders(str(tmp_path), "ChestXRay", "grayscaled", 4, 3, cache="host")
    assert str(e.value) == "cache must be one of ('none', 'device') (cache='host')"
    with pytest.raises(ValueError) as e:
        td.default_loader(ns(preprocess="grayscaled", train_cache="host"), cfg, "cuda", "training", 4, shuffle=True)
    assert str(e.value) == "train_cache must be one of ('none', 'device') (train_cache='host')"
