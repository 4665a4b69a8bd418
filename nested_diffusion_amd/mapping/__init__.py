"""Mapping network: ViT prefix blocks + mapping MLPs -> latent conditions (guiding predictions).

Mirrors Diffusion.compute_guiding_prediction (classification_train_separately.py:330-348), mapping/models/mlp.py::Classifier and the timm
0.4.12 vit_base_patch16_224 pieces it calls.  All arithmetic runs in libnd_hip.so.  One module per job: mlp (Classifier), vit
(VisionTransformer, forward and backward chain, and the refusals the gradient paths share), conditioner (GuidingConditioner and the
attack target on it), checkpoint (the restricted unpickler and the readers of the reference's checkpoint files)."""
from .checkpoint import (_module_tree_state_dict, _skeleton_pickle_module, _SkeletonUnpickler, _to_state_dict, load_checkpoint_object,
                         load_conditioner, load_pickled)
from .conditioner import ConditionerTarget, GuidingConditioner
from .mlp import Classifier
from .vit import LN_EPS, VisionTransformer, check_backward_tokens, require_fp32_split
