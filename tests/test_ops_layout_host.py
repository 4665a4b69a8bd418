"""The layout of nested_diffusion_amd.ops: one module per job, every name callers use on the package, one stream lookup, and the
constants the wrappers restate equal to the header's.  Host only: no GPU, no library."""
import importlib
import inspect
import pathlib
import re
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
PKG = ROOT / "nested_diffusion_amd"

PUBLIC = [
    "ACT", "APGD_IMPROVED", "APGD_NOT_PRED", "APGD_RESTORE", "ATTENTION_BWD_MAX_TOKENS", "ApgdState", "BN_EPS", "BN_MOMENTUM", "COLSUM_CHUNK",
    "CwState", "L2_MAX_PARTS", "LINEAR_BWD_MAX_M", "ND_ACT_GELU", "ND_ACT_NONE", "ND_ACT_RELU", "ND_ACT_SOFTPLUS", "PackedWeight",
    "SQUARE_ACCEPT", "SQUARE_ACTIVE", "SUMSQ_CHUNK", "SplitMatrix", "SquareState", "adam_step", "adamw_step", "aggregate", "apgd_control",
    "apgd_random_start", "apgd_update", "attention", "attention_grad", "attention_images", "attention_split", "bias_grad_adam",
    "bn_train_backward", "bn_train_forward", "clip_adam", "colsum_adamw", "cw_attack_space", "cw_b_half", "cw_control", "cw_model_space",
    "cw_update", "ensemble_xent_grad", "gelu_grad_split", "gelu_split", "gemm_bias_act", "gemm_split", "gemm_split_qkv", "gemm_tn_adamw",
    "gemm_tn_plan", "join_rows", "l2_random_start", "l2_step", "layernorm", "layernorm_grad", "layernorm_split", "layernorm_wgrad_adamw",
    "linear", "linear_grad_input", "linear_wgrad_adam", "linear_wgrad_plan", "linf_random_start", "linf_step", "margin_head_grad", "mse_grad",
    "patchify", "patchify_split", "qkv_images_supported", "qsample", "report", "sample_stats", "softmax_rows", "split_rows", "square_accept",
    "square_commit", "square_init", "square_propose", "sumsq", "sumsq_plan", "unpatchify", "xent_head_grad"]
PRIVATE = ["_f32", "_stream", "_workspace", "_ws_cache"]


def test_every_name_is_on_the_package_and_defined_in_one_submodule():
    from nested_diffusion_amd import ops
    assert len(PUBLIC) == 81 and len(set(PUBLIC)) == 81
    for name in PUBLIC + PRIVATE:
        assert hasattr(ops, name), name
        obj = getattr(ops, name)
        if inspect.isfunction(obj) or inspect.isclass(obj):
            assert obj.__module__.startswith("nested_diffusion_amd.ops."), (name, obj.__module__)      # a submodule, not the package
            assert getattr(sys.modules[obj.__module__], name) is obj, name


def test_the_package_file_only_imports():
    import ast
    body = ast.parse((PKG / "ops" / "__init__.py").read_text()).body
    assert isinstance(body[0], ast.Expr) and isinstance(body[0].value, ast.Constant)                   # the docstring
    assert all(isinstance(node, ast.ImportFrom) for node in body[1:])
    assert not any(alias.name == "*" for node in body[1:] for alias in node.names)


def test_ws_cache_is_the_dict_workspace_fills():
    from nested_diffusion_amd import ops
    base = importlib.import_module("nested_diffusion_amd.ops._base")
    assert ops._ws_cache is base._ws_cache
    assert ops._workspace is base._workspace and ops._workspace.__globals__["_ws_cache"] is ops._ws_cache


def test_the_stream_lookup_is_written_once():
    hits = [str(p.relative_to(PKG)) for p in sorted(PKG.rglob("*.py")) for line in p.read_text().splitlines() if ".cuda_stream" in line]
    assert hits == ["_lib.py"], hits


def _defines(path: pathlib.Path) -> dict:
    """Every `#define NAME <integer>` of a C source, read with one regular expression."""
    return {name: int(value, 0) for name, value in re.findall(r"^\s*#\s*define\s+(\w+)\s+\(?(0[xX][0-9a-fA-F]+|\d+)\)?\s*(?:/[/*].*)?$",
                                                              path.read_text(), re.M)}


def test_restated_constants_equal_the_headers():
    from nested_diffusion_amd import ops
    header = _defines(ROOT / "include" / "nested_diffusion.h")
    for name, macro in (("LINEAR_BWD_MAX_M", "ND_LINEAR_BWD_MAX_M"), ("L2_MAX_PARTS", "ND_L2_MAX_PARTS"), ("COLSUM_CHUNK", "ND_COLSUM_CHUNK"),
                        ("SUMSQ_CHUNK", "ND_SUMSQ_CHUNK"), ("APGD_NOT_PRED", "ND_APGD_NOT_PRED"), ("APGD_IMPROVED", "ND_APGD_IMPROVED"),
                        ("APGD_RESTORE", "ND_APGD_RESTORE"), ("SQUARE_ACTIVE", "ND_SQUARE_ACTIVE"), ("SQUARE_ACCEPT", "ND_SQUARE_ACCEPT"),
                        ("ND_ACT_NONE", "ND_ACT_NONE"), ("ND_ACT_SOFTPLUS", "ND_ACT_SOFTPLUS"), ("ND_ACT_RELU", "ND_ACT_RELU"),
                        ("ND_ACT_GELU", "ND_ACT_GELU")):
        assert macro in header, macro
        assert getattr(ops, name) == header[macro], (name, getattr(ops, name), header[macro])
    unit = _defines(PKG / "csrc" / "nd_vit_grad.hip")
    assert ops.ATTENTION_BWD_MAX_TOKENS == unit["ATB_NMAX"]
