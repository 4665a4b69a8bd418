"""The tile order of the LDS-tiled kernels (csrc/nd_tile.hpp) walked on the host: tools/check_tile_order.hip built for the host alone
and run -- nd_xcd_run is a bijection that hands every XCD one contiguous run, nd_tile_decode visits every whole tile and every
(remainder tile, k-slab) once, the slab ranges of a tile partition its K-steps.  No GPU is touched."""
import os
import subprocess

import pytest

from nested_diffusion_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_order_on_the_host(tmp_path):
    try:
        hipcc = build._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    exe = str(tmp_path / "check_tile_order")
    cc = subprocess.run([hipcc, "--cuda-host-only", "-O1", "-std=c++17", os.path.join(ROOT, "tools", "check_tile_order.hip"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("0 failed"), run.stdout + run.stderr
