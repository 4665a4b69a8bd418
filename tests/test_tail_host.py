"""Argument rejections of the aggregation, report, image and noise operators (csrc/nd_report.hip, csrc/nd_image.hip, csrc/nd_rng.hip).
Every one is decided on the host before any launch, so this runs without a GPU: the tensor arguments are small dummy non-NULL
addresses that are never dereferenced.  Each call must return nonzero and leave a message in nd_last_error() that names the
offending argument with the value it had (the keyword beside each case).  The limits are the
kernels' fixed array sizes and packed counter fields: ND_AGG_MAX_C = 16 classes, ND_STATS_MAXS = 4096 samples, ND_REPORT_MAXBINS = 64
bins, member < 255 (8 bits), trial < 65535 (16 bits), class quad < 256 (8 bits)."""
import pytest

P = 0x1000                      # a dummy device address
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    from nested_diffusion_amd import _lib, build
    build.build()               # hipcc cross-compiles for gfx950 without a GPU
    return _lib.load()


def clear(lib):
    """leave a known, unrelated text in nd_last_error(), so that a rejection which sets no message of its own is noticed"""
    assert lib.nd_philox_normal(None, 1, 1, 1, 1, 1, 0, 0, 0, None) != 0
    assert lib.nd_last_error() == b"out_dev is NULL"


# name: (call, what its message must contain)
REJECTIONS = {
    # nd_aggregate(samples, prob, vote, probs, S, B, C, temperature, stream)
    "aggregate_C17": (lambda L: L.nd_aggregate(P, P, P, P, 2, 3, 17, 0.1737, None), b"C=17"),
    "aggregate_S0": (lambda L: L.nd_aggregate(P, P, P, P, 0, 3, 2, 0.1737, None), b"S=0"),
    "aggregate_temp0": (lambda L: L.nd_aggregate(P, P, P, P, 2, 3, 2, 0.0, None), b"temperature=0"),
    "aggregate_temp_nan": (lambda L: L.nd_aggregate(P, P, P, P, 2, 3, 2, NAN, None), b"temperature=nan"),
    # nd_sample_stats(probs, piw, var, S, B, C, q_lo, q_hi, stream)
    "stats_S4097": (lambda L: L.nd_sample_stats(P, P, P, 4097, 3, 2, 0.025, 0.975, None), b"S=4097"),
    "stats_S0": (lambda L: L.nd_sample_stats(P, P, P, 0, 3, 2, 0.025, 0.975, None), b"S=0"),
    "stats_q_order": (lambda L: L.nd_sample_stats(P, P, P, 8, 3, 2, 0.75, 0.25, None), b"q_lo=0.75, q_hi=0.25"),
    "stats_q_hi_above_1": (lambda L: L.nd_sample_stats(P, P, P, 8, 3, 2, 0.5, 1.5, None), b"q_hi=1.5"),
    "stats_q_lo_nan": (lambda L: L.nd_sample_stats(P, P, P, 8, 3, 2, NAN, 0.975, None), b"q_lo=nan"),
    "stats_q_hi_nan": (lambda L: L.nd_sample_stats(P, P, P, 8, 3, 2, 0.025, NAN, None), b"q_hi=nan"),
    # nd_report(piw, var, pm, vote, target, out, N, C, temperature, n_bins, stream)
    "report_C17": (lambda L: L.nd_report(P, P, P, P, P, P, 5, 17, 0.1737, 10, None), b"C=17"),
    "report_bins0": (lambda L: L.nd_report(P, P, P, P, P, P, 5, 2, 0.1737, 0, None), b"n_bins=0"),
    "report_bins65": (lambda L: L.nd_report(P, P, P, P, P, P, 5, 2, 0.1737, 65, None), b"n_bins=65"),
    "report_N0": (lambda L: L.nd_report(P, P, P, P, P, P, 0, 2, 0.1737, 10, None), b"N=0"),
    "report_temp0": (lambda L: L.nd_report(P, P, P, P, P, P, 5, 2, 0.0, 10, None), b"temperature=0"),
    "report_temp_negative": (lambda L: L.nd_report(P, P, P, P, P, P, 5, 2, -0.25, 10, None), b"temperature=-0.25"),
    # nd_img_resize_bilinear(x, out, B, C, Hi, Wi, Ho, Wo, crop, crop_size, stream)
    "resize_Ho0": (lambda L: L.nd_img_resize_bilinear(P, P, 1, 3, 7, 5, 0, 4, None, 0, None), b"Ho=0"),
    "resize_Wi0": (lambda L: L.nd_img_resize_bilinear(P, P, 1, 3, 7, 0, 4, 4, None, 0, None), b"Wi=0"),
    "resize_crop_above_min_side": (lambda L: L.nd_img_resize_bilinear(P, P, 1, 3, 7, 5, 7, 5, P, 6, None), b"crop_size=6"),
    "resize_crop0": (lambda L: L.nd_img_resize_bilinear(P, P, 1, 3, 7, 5, 7, 5, P, 0, None), b"crop_size=0"),
    # nd_img_cover(x, B, C, H, W, rects, n_rects, side, stream)
    "cover_side_above_H": (lambda L: L.nd_img_cover(P, 1, 3, 5, 9, P, 1, 6, None), b"side=6"),
    "cover_side_negative": (lambda L: L.nd_img_cover(P, 1, 3, 5, 9, P, 1, -1, None), b"side=-1"),
    # nd_img_contrast(x, out, mean_ws, B, per_image, k, stream)
    "contrast_per0": (lambda L: L.nd_img_contrast(P, P, P, 2, 0, 1.7, None), b"per_image=0"),
    # nd_philox_normal(out, K, T, B, mc, C, seed, batch_counter, first_image, stream)
    "philox_K256": (lambda L: L.nd_philox_normal(P, 256, 1, 1, 1, 1, 0, 0, 0, None), b"n_members=256"),
    "philox_mc65536": (lambda L: L.nd_philox_normal(P, 1, 1, 1, 65536, 1, 0, 0, 0, None), b"mc=65536"),
    "philox_C1025": (lambda L: L.nd_philox_normal(P, 1, 1, 1, 1, 1025, 0, 0, 0, None), b"C=1025"),
}


@pytest.mark.parametrize("name", sorted(REJECTIONS))
def test_rejected_before_any_launch(lib, name):
    call, keyword = REJECTIONS[name]
    clear(lib)
    assert call(lib) != 0, name
    assert keyword in lib.nd_last_error(), (name, lib.nd_last_error())     # this call's message: it names the argument and its value


def test_softmax_rows_rejects_zero_rows(lib):
    clear(lib)
    assert lib.nd_softmax_rows(P, P, 0, 4, None) != 0
    assert b"rows=0" in lib.nd_last_error()


def test_null_tensors_are_reported_as_such(lib):
    """a NULL tensor is reported before any shape (the GPU tests rely on the shapes alone deciding the rejections above)"""
    for rc in (lib.nd_aggregate(None, P, P, P, 2, 3, 2, 0.1737, None), lib.nd_sample_stats(P, None, P, 8, 3, 2, 0.025, 0.975, None),
               lib.nd_report(P, P, P, P, P, None, 5, 2, 0.1737, 10, None), lib.nd_softmax_rows(None, P, 3, 4, None),
               lib.nd_img_contrast(P, P, None, 2, 16, 1.7, None), lib.nd_img_resize_bilinear(P, None, 1, 3, 7, 5, 4, 4, None, 0, None),
               lib.nd_img_cover(P, 1, 3, 5, 9, None, 1, 2, None)):
        assert rc != 0 and b"NULL" in lib.nd_last_error(), lib.nd_last_error()
