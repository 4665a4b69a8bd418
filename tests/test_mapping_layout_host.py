"""The layout of nested_diffusion_amd.mapping: one module per job, every name callers use on the package, and the facts about the models
that are written once in the package (the padded width of lin1, the call that forms the noise schedule).  Host only: no GPU, no library."""
import ast
import inspect
import pathlib
import re
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
PKG = ROOT / "nested_diffusion_amd"

PUBLIC = ["Classifier", "ConditionerTarget", "GuidingConditioner", "LN_EPS", "VisionTransformer", "check_backward_tokens",
          "load_checkpoint_object", "load_conditioner", "load_pickled", "require_fp32_split"]
PRIVATE = ["_SkeletonUnpickler", "_module_tree_state_dict", "_skeleton_pickle_module", "_to_state_dict"]      # tests and tools import these


def test_every_name_is_on_the_package_and_defined_in_one_submodule():
    from nested_diffusion_amd import mapping
    assert len(PUBLIC) == 10 and len(set(PUBLIC + PRIVATE)) == 14
    for name in PUBLIC + PRIVATE:
        assert hasattr(mapping, name), name
        obj = getattr(mapping, name)
        if inspect.isfunction(obj) or inspect.isclass(obj):
            assert obj.__module__.startswith("nested_diffusion_amd.mapping."), (name, obj.__module__)      # a submodule, not the package
            assert getattr(sys.modules[obj.__module__], name) is obj, name
    assert mapping.LN_EPS == sys.modules["nested_diffusion_amd.mapping.vit"].LN_EPS == 1e-6
    # no submodule shares its name with something callers take from the package
    subs = {p.stem for p in (PKG / "mapping").glob("*.py")} - {"__init__"}
    assert subs == {"mlp", "vit", "conditioner", "checkpoint"} and not subs & set(PUBLIC + PRIVATE)
    # the path the unpickler's refusal names still resolves
    assert sys.modules["nested_diffusion_amd"].mapping._SkeletonUnpickler is mapping._SkeletonUnpickler


def test_the_package_file_only_imports():
    body = ast.parse((PKG / "mapping" / "__init__.py").read_text()).body
    assert isinstance(body[0], ast.Expr) and isinstance(body[0].value, ast.Constant)                   # the docstring
    assert len(body) > 1 and all(isinstance(node, ast.ImportFrom) for node in body[1:])
    assert not any(alias.name == "*" for node in body[1:] for alias in node.names)


def _files_matching(pattern: str):
    return sorted({str(p.relative_to(PKG)) for p in PKG.rglob("*.py") if re.search(pattern, p.read_text())})


def test_the_padded_width_and_the_schedule_call_are_written_once():
    assert _files_matching(r"LIN1_K\s*=\s*\d") == ["latent_model.py"]
    assert _files_matching(r"make_beta_schedule\(") == ["diffusion_utils.py"]
