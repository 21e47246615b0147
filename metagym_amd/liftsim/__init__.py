"""Batched LiftSim elevator dispatch on the GPU (mirrors metagym/liftsim/__init__.py: id liftsim-v0)."""
from .liftsim_env import (DEFAULTS, ElevatorState, LiftSim, MansionAttribute, MansionState, custom_tables, read_config,
                          resolve_config)
from .policy import LiftPolicy, LiftPolicyState, LiftRecurrentPolicy

__all__ = ["DEFAULTS", "ElevatorState", "LiftPolicy", "LiftPolicyState", "LiftRecurrentPolicy", "LiftSim", "MansionAttribute",
           "MansionState", "custom_tables", "read_config", "resolve_config"]
