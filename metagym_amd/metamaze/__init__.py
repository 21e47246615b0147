"""Batched MetaMaze (mirrors metagym/metamaze/__init__.py: ids meta-maze-2D-v0,
meta-maze-discrete-3D-v0, meta-maze-continuous-3D-v0)."""
from .expert import MazeDistanceField, distance_field_reference, expert_action_reference
from .maze_env import MetaMaze2D, MetaMazeDiscrete3D, MetaMazeContinuous3D, rollout_obs_steps
from .maze_task import MAZE_TASK_MANAGER, DeviceTaskTable, MazeTaskManager, MazeTaskSampler, TaskConfig
from .policy import Maze3DPolicy, Maze3DPolicyState, Maze3DSteerPolicy, MazePolicy, MazePolicyRollout, MazePolicyState
from .policy_net import MazePolicyNet, log_prob

__all__ = ["MetaMaze2D", "MetaMazeDiscrete3D", "MetaMazeContinuous3D", "MazeTaskSampler", "MazeTaskManager",
           "MAZE_TASK_MANAGER", "TaskConfig", "DeviceTaskTable", "rollout_obs_steps", "MazePolicy", "MazePolicyState",
           "MazePolicyRollout", "MazeDistanceField", "distance_field_reference", "expert_action_reference", "Maze3DPolicy",
           "Maze3DSteerPolicy", "Maze3DPolicyState", "MazePolicyNet", "log_prob"]
