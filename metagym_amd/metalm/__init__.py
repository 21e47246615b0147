"""MetaLM sequence batches generated on the GPU (mirrors metagym/metalm/__init__.py: id meta-lm-v0)."""
from .metalm import MetaLM, default_element_capacity

__all__ = ["MetaLM", "default_element_capacity"]
