"""Batched K-armed Bernoulli bandits on the GPU (mirrors metagym/bandits/__init__.py: id bandits-v0)."""
from .bandits_env import DISTRIBUTIONS, Bandits, classical_lo_hi
from .learner import BanditLearner, BanditLearnerState, BanditsLearnerRollout, gittins_index_table, log32
from .policy import BanditPolicy, BanditPolicyState, BanditsPolicyRollout
from .policy_net import BanditPolicyNet, log_prob

__all__ = ["Bandits", "DISTRIBUTIONS", "classical_lo_hi", "BanditPolicy", "BanditPolicyState", "BanditsPolicyRollout",
           "BanditLearner", "BanditLearnerState", "BanditsLearnerRollout", "gittins_index_table", "log32", "BanditPolicyNet", "log_prob"]
