"""Batched K-armed Bernoulli bandits on the GPU (mirrors metagym/bandits/__init__.py: id bandits-v0)."""
from .bandits_env import DISTRIBUTIONS, Bandits, classical_lo_hi

__all__ = ["Bandits", "DISTRIBUTIONS", "classical_lo_hi"]
