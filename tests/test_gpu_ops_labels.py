"""The one label check of nested_diffusion_amd.ops at the six wrappers that take labels, at the smallest shapes (B = 2, C = 3): the
labels arrive as int64 on the device whatever they were, a wrong shape is refused, the range check runs only where check_labels asks
for it, and the three bookkeeping wrappers read nothing back."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, C = 2, 3
LOGITS = torch.tensor([[0.5, -1.25, 2.0], [1.5, 0.25, -0.75]])
LABELS = torch.tensor([2, 1])
CHECKED = ("xent_head_grad", "margin_head_grad", "ensemble_xent_grad")        # take check_labels; the NaN is in result [1]: loss / margin
UNCHECKED = ("apgd_control", "square_accept", "cw_control")                   # per-image bookkeeping: never range-check, never read back


def head_w(E):
    return (torch.arange(C * E, dtype=torch.float32).reshape(C, E) / 4 - 1).to(DEV)


def zeroed(state):
    """Every field the control kernels may leave unwritten holds a known value, so that two runs compare bit for bit."""
    for name, _, _ in state.fields:
        getattr(state, name).zero_()
    return state


def run(name, labels, **kw):
    """The wrapper on the module's logits with `labels`, its other arguments as its own tests build them; every result on the host."""
    from nested_diffusion_amd import ops
    logits, per_row = LOGITS.to(DEV), torch.tensor([1.5, 0.5], device=DEV)
    if name == "xent_head_grad":
        out = ops.xent_head_grad(logits, labels, head_w(1), **kw)                            # E = 1: the sweep of test_gpu_grad_edges
    elif name == "margin_head_grad":
        out = ops.margin_head_grad(logits, labels, per_row, head_w(4), 0.5, **kw)            # E = 4: test_margin_head_ragged_trips
    elif name == "ensemble_xent_grad":
        out = ops.ensemble_xent_grad(logits[None], labels, **kw)                             # K = 1
    elif name == "apgd_control":
        st = zeroed(ops.ApgdState(B, 4, DEV))
        flags = ops.apgd_control(logits, labels, per_row, st, -1, 0, 0.75, step0=0.25)
        assert flags is st.flags
        out = [getattr(st, n) for n, _, _ in st.fields]
    elif name == "square_accept":
        st = zeroed(ops.SquareState(B, DEV))
        flags = ops.square_accept(logits, labels, st, -1)
        assert flags is st.flags
        out = [getattr(st, n) for n, _, _ in st.fields]
    else:
        st = zeroed(ops.CwState(torch.zeros(B, 4, device=DEV)))
        st.sq_rec.copy_(torch.tensor([0.25, 0.5])), st.sq_x0.copy_(torch.tensor([1.0, 4.0])), st.best_norm.fill_(float("inf"))
        loss = ops.cw_control(logits, labels, per_row, torch.tensor([0.75, -0.5], device=DEV), st, 0.25)
        assert loss is st.loss
        out = [getattr(st, n) for n, _, _ in st.fields]
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("name", CHECKED + UNCHECKED)
def test_int32_host_labels_give_the_bits_of_int64_device_labels(name):
    want = run(name, LABELS.to(DEV))
    got = run(name, LABELS.to(torch.int32))
    assert len(got) == len(want) >= 2
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(bits(g), bits(w))
    assert all(bool(t.isfinite().all()) for t in want if t.dtype == torch.float32 and name != "cw_control")


@pytest.mark.parametrize("name", CHECKED + UNCHECKED)
def test_labels_of_another_length_are_refused(name):
    with pytest.raises(ValueError, match="labels"):
        run(name, torch.zeros(B + 1, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize("name", CHECKED)
def test_the_range_check_runs_only_when_asked(name):
    """A label C: refused with the check on.  With it off the kernel's own guard answers: a NaN loss (margin) in that row alone."""
    bad = torch.tensor([1, C], device=DEV)
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 3\)"):
        run(name, bad)
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 3\)"):
        run(name, bad, check_labels=True)
    row = run(name, bad, check_labels=False)[1]
    assert row.shape == (B,) and bool(row[1].isnan()) and bool(row[0].isfinite())


@pytest.mark.parametrize("name", UNCHECKED)
def test_bookkeeping_wrappers_read_nothing_back(name):
    labels = LABELS.to(DEV)
    run(name, labels)                                            # the library is loaded and the states' allocator is warm
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        sync_free_call(name, labels)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()


def sync_free_call(name, labels):
    """The wrapper's call alone, on device arguments made by fills (no upload, which would itself synchronise)."""
    from nested_diffusion_amd import ops
    logits, per_row = torch.full((B, C), 0.5, device=DEV), torch.full((B,), 1.5, device=DEV)
    if name == "apgd_control":
        ops.apgd_control(logits, labels, per_row, ops.ApgdState(B, 4, DEV), -1, 0, 0.75, step0=0.25)
    elif name == "square_accept":
        ops.square_accept(logits, labels, ops.SquareState(B, DEV), -1)
    else:
        ops.cw_control(logits, labels, per_row, per_row, ops.CwState(torch.zeros(B, 4, device=DEV)), 0.25)
