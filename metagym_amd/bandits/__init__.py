"""Batched K-armed Bernoulli bandits on the GPU (mirrors metagym/bandits/__init__.py: id bandits-v0)."""
from .bandits_env import DISTRIBUTIONS, Bandits, classical_lo_hi
from .policy import BanditPolicy, BanditPolicyState, BanditsPolicyRollout

__all__ = ["Bandits", "DISTRIBUTIONS", "classical_lo_hi", "BanditPolicy", "BanditPolicyState", "BanditsPolicyRollout"]
