"""Batched Quadrotor (mirrors metagym/quadrotor/__init__.py: id 'quadrotor-v0')."""
from .env import Quadrotor, DEFAULT_SIM_CONFIG
from .policy import PolicyRollout, QuadrotorPolicy, QuadrotorPolicyState, QuadrotorRecurrentPolicy
from .tasks import QuadrotorTaskTable, sample_tasks

__all__ = ["Quadrotor", "DEFAULT_SIM_CONFIG", "QuadrotorTaskTable", "sample_tasks", "QuadrotorPolicy", "PolicyRollout",
           "QuadrotorRecurrentPolicy", "QuadrotorPolicyState"]
