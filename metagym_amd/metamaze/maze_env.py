"""Batched MetaMaze envs — host-side mirror of metagym/metamaze/envs/maze_env.py:16,85,155.

Same class names, constructor arguments, `set_task()` / `reset()` / `step()` surface and the same
observation dtypes (2-D: float32 window; 3-D: int32 [H,V,3] image whose values exceed 255), but
every call advances `num_envs` mazes with one launch of the gfx950 kernels behind
`mg_maze2d_step` / `mg_maze3d_step` (include/metagym_hip.h, metagym_amd/csrc/maze.hip) and returns
torch-ROCm tensors of shape [num_envs, ...].

Batched extensions
  * `set_task(task)` gives every env the same TaskConfig; `set_task([t0, t1, ...], task_ids=ids)`
    uploads a table of T tasks (all the same size n) and env e plays task `ids[e]`
    (default e mod T).
  * the reference raises when step() is called on a finished episode (maze_env.py:60-61); per-lane
    exceptions do not exist on a GPU, so either reset the finished envs with `reset(mask=done)` or
    construct the env with `auto_reset=True` (finished envs restart inside the same launch and the
    returned observation is the first one of the next episode).
  * rendering (`enable_render`, pygame god-view) is out of scope; the argument is accepted and ignored.

Size limits (include/metagym_hip.h)
  * 3 <= n <= 255 for every env. Above n = 181 (more than 32 768 cells) the int16 SURVIVAL food list cannot index the table:
    the env passes none and MetaMaze2D keeps its SURVIVAL arrays by cell instead of by slot (exact, slower).
  * 3-D: a ray keeps at most 127 translucent cells; min(2n+1, 2 * int(max_vision_range / cell size) + 5) above 127 (n >= 64 with
    a cell size <= max_vision_range / 62) raises ValueError at set_task. The renderer's LDS must fit 160 KiB (n <= 124 at cell
    size 2 and a small frame), else the first launch raises MetaGymHipError naming the bytes.
"""

import numpy as np
import torch

from .. import _lib, _policy
from ..spaces import Box, Discrete
from .maze_task import MAZE_TASK_MANAGER, DeviceTaskTable, TaskConfig, forget_when_freed  # noqa: F401  (TaskConfig re-exported like the reference's maze_env)

PI = 3.1415926                      # dynamics.py:6
DISCRETE_ACTIONS = [(-1, 0), (1, 0), (0, -1), (0, 1)]   # maze_env.py:14
TASK_TYPES = {"ESCAPE": 0, "SURVIVAL": 1}
MAX_RAY_RECORDS = 127              # translucent cells one ray of the 3-D renderer can record (mg_maze_view.max_ray_records)


FOOD_LIST_MAX_CELLS = 32768        # mg_maze_tasks.food_cells / cell_slot hold int16 cell indices: n * n <= 32 768 (n <= 181)


def food_lists(food_rewards, food_interval, by_slot):
    """The optional SURVIVAL accelerator of mg_maze_tasks (include/metagym_hip.h) for a [T, n*n] task table, built with tensor ops
    on the table's own device: `food_cells` (per task, the cells that can ever hold food — interval > 0 or food > 1e-2 — in
    ascending order, int16 [T, max_food]), `n_food` (int32 [T]), `max_food`, and with `by_slot` the slot layout of the 2-D kernel:
    `cell_slot` (int16 [T, n*n], the inverse map) and the listed cells' values slot-major, `slot_food` / `slot_interval`
    ([max_food, T]). None when the table has more than FOOD_LIST_MAX_CELLS cells: int16 cannot index them (the library refuses
    such lists), and the kernels sweep every cell instead — exact, only slower."""
    import torch
    T, nn = food_rewards.shape
    if nn > FOOD_LIST_MAX_CELLS:
        return None
    dev = food_rewards.device
    can = (food_interval > 0) | (food_rewards > 1.0e-2)                                      # [T, nn]
    n_food = can.sum(dim=1).to(torch.int32)
    max_food = max(1, int(n_food.max().item()))
    order = torch.argsort((~can).to(torch.int8), dim=1, stable=True)[:, :max_food]   # food cells first, ascending
    out = dict(food_cells=order.to(torch.int16).contiguous(), n_food=n_food.contiguous(), max_food=max_food)
    if by_slot:
        # the list once more for the lane-per-env kernel (mg_maze_tasks.cell_slot / slot_food / slot_interval): the inverse
        # map cell -> slot, and the listed cells' task values slot-major, [max_food][T]
        listed = torch.arange(max_food, device=dev).unsqueeze(0) < n_food.unsqueeze(1)              # [T, max_food]
        # cells outside the list: -1 when the task's value there is exactly 0.0 (the kernel then reads nothing for them), -2 when
        # it is a nonzero value <= 1e-2 (never eaten, never renewed, but part of the 2-D observation: read from the task)
        slot = torch.where(food_rewards != 0.0, torch.full((T, nn), -2, dtype=torch.int16, device=dev),
                           torch.full((T, nn), -1, dtype=torch.int16, device=dev))
        ks = torch.arange(max_food, device=dev, dtype=torch.int16).unsqueeze(0).expand(T, max_food)
        # only the LISTED entries of a row are written: a task with n_food < max_food has non-food cells in the tail of its
        # `order` row, and those keep their -1 / -2 (a -1 there would hide a nonzero crumb from the observation)
        slot.scatter_(1, order, torch.where(listed, ks, slot.gather(1, order)))        # (a row of `order` holds distinct cells)
        out.update(cell_slot=slot.contiguous(), slot_food=torch.gather(food_rewards, 1, order).t().contiguous(),
                   slot_interval=torch.gather(food_interval, 1, order).t().contiguous())
    return out


def rollout_obs_steps(n_steps, obs_every):
    """The steps (0-based, ascending) of a `rollout` of `n_steps` steps that leave an observation: `obs_every` 0 = the last
    step only; k >= 1 = every step t with (t + 1) % k == 0, and always the last one (never twice). The kernels apply the same
    rule (csrc/maze_core.h rollout_records)."""
    n_steps, obs_every = int(n_steps), int(obs_every)
    if n_steps < 1:
        raise ValueError("a rollout needs at least one step (got %d)" % n_steps)
    if obs_every < 0:
        raise ValueError("obs_every must be 0 (the last step only) or k >= 1 (every k-th step), got %d" % obs_every)
    return [t for t in range(n_steps) if t == n_steps - 1 or (obs_every > 0 and (t + 1) % obs_every == 0)]


class _MazeBatch(object):
    """State, task table and launch plumbing shared by the three envs."""

    def __init__(self, num_envs, device, max_steps, task_type, auto_reset):
        assert task_type in TASK_TYPES, "task_type must be ESCAPE or SURVIVAL"
        self._lib = _lib.load()
        self.num_envs = int(num_envs)
        self.device = _lib.canonical_device(device)
        if self.device.type != "cuda":
            raise _lib.MetaGymHipError("metagym_amd runs on an AMD GPU only (got device %r); there is no CPU "
                                       "path" % (device,))
        self.max_steps = int(max_steps)
        self.task_type = task_type
        self._tt = TASK_TYPES[task_type]
        self.auto_reset = bool(auto_reset)
        self.need_set_task = True
        self.need_reset = True
        self._tasks_c = None
        self._goal_field = None
        self._expert_action = None
        N, dev = self.num_envs, self.device
        self._reward = torch.zeros(N, dtype=torch.float32, device=dev)
        self._reward64 = torch.zeros(N, dtype=torch.float64, device=dev)
        self._done = torch.zeros(N, dtype=torch.bool, device=dev)

    # ------------------------------------------------------------------ tasks
    def set_task(self, task_config, task_ids=None):
        """task_config: one TaskConfig, a list of T TaskConfigs (uploaded once), or a DeviceTaskTable from
        `MazeTaskManager.sample_tasks_device` (already on the GPU). Env e plays task task_ids[e]
        (default e mod T)."""
        N, dev = self.num_envs, self.device
        if isinstance(task_config, DeviceTaskTable):
            n, T = task_config.n, task_config.n_tasks
            assert all(v.device == dev or (v.device.type == dev.type and (v.device.index or 0) == (dev.index or 0))
                       for v in task_config.tensors.values()), "task table lives on another device"
            self._check_table(n, float(task_config.cell_size))       # before anything of this env changes
            self._task_t = task_config.tensors
            self.tasks = task_config
            self._min_cell_size = float(task_config.cell_size)
            self._uniform_cell_size = float(task_config.cell_size)       # one sampler configuration: one cell size
            host = task_config.tensors
        else:
            tasks = [task_config] if isinstance(task_config, tuple) and hasattr(task_config, "cell_walls") else list(task_config)
            assert len(tasks) >= 1
            n = int(np.shape(tasks[0].cell_walls)[0])
            T = len(tasks)
            for t in tasks:   # maze_base.py:35-38
                assert np.shape(t.cell_walls) == (n, n), "all tasks of one batch must have the same size"
                assert 0 < t.agent_height < t.wall_height, "the agent height must be > 0 and < wall height"
                assert np.shape(t.cell_walls) == np.shape(t.cell_texts), "the dimension of walls must be equal to textures"
            self._check_table(n, min(float(t.cell_size) for t in tasks))   # before anything of this env changes
            host = dict(
                start=np.asarray([t.start for t in tasks], np.int32).reshape(T, 2),
                goal=np.asarray([t.goal for t in tasks], np.int32).reshape(T, 2),
                walls=np.clip(np.asarray([t.cell_walls for t in tasks]), -1, 1).astype(np.int8).reshape(T, n * n),
                texts=np.asarray([t.cell_texts for t in tasks]).astype(np.uint8).reshape(T, n * n),
                food_rewards=np.asarray([t.food_rewards for t in tasks], np.float64).reshape(T, n * n),
                food_interval=np.asarray([t.food_interval for t in tasks], np.int32).reshape(T, n * n),
                scalars=np.asarray([[t.cell_size, t.wall_height, t.agent_height, t.initial_life, t.max_life,
                                     t.step_reward, t.goal_reward, 0.0] for t in tasks], np.float64))
            assert int(host["texts"].max()) < MAZE_TASK_MANAGER.n_texts, "cell_texts refers to a missing texture"
            self._task_t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in host.items()}
            forget_when_freed(self._task_t["scalars"])       # this env's own upload: forgotten when it is freed
            self.tasks = tasks
            self._min_cell_size = min(float(t.cell_size) for t in tasks)
            sizes = set(float(t.cell_size) for t in tasks)
            self._uniform_cell_size = sizes.pop() if len(sizes) == 1 else 0.0   # mg_maze_view.uniform_cell_size: 0 = tasks differ
        nn = n * n
        self.n = n
        # (the library's address-keyed memory of a checked (table, uniform_cell_size) pair is dropped when the table's scalar rows
        # are freed — forget_when_freed, registered where the table is created — never by an env: envs may share a table)
        c = _lib.MazeTasks()
        c.n, c.n_tasks = n, T
        for k in host:
            setattr(c, k, self._task_t[k].data_ptr())
        # compact list of the cells that can ever hold food (exact shortcut for the SURVIVAL sweeps, see
        # include/metagym_hip.h); built with device ops so a DeviceTaskTable never visits the host. The list and the slot map
        # hold int16 cell indices: a table with more than 32 768 cells gets neither (the kernels then sweep every cell) and
        # keeps its SURVIVAL arrays by cell
        lists = food_lists(self._task_t["food_rewards"], self._task_t["food_interval"], self._BY_SLOT)
        self._by_slot = lists is not None and "cell_slot" in lists
        if lists is not None:
            self._food_cells_t, self._n_food_t, self._max_food = lists["food_cells"], lists["n_food"], lists["max_food"]
            c.food_cells, c.n_food, c.max_food = self._food_cells_t.data_ptr(), self._n_food_t.data_ptr(), self._max_food
        if self._by_slot:
            self._cell_slot_t, self._slot_food_t, self._slot_interval_t = (lists["cell_slot"], lists["slot_food"],
                                                                           lists["slot_interval"])
            c.cell_slot, c.slot_food, c.slot_interval = (self._cell_slot_t.data_ptr(), self._slot_food_t.data_ptr(),
                                                         self._slot_interval_t.data_ptr())
        self._tasks_c = c
        self._goal_field = None                                      # the cached goal field was the previous table's
        if self._uniform_cell_size > 0.0:
            # the promise mg_maze_view.uniform_cell_size makes about THIS table, checked by the library against the uploaded
            # cell_size column (synchronous, once per set_task; a hipGraph capture of step() later finds the pair checked)
            _lib.check(self._lib.mg_maze_check_uniform_cell_size(c, self._uniform_cell_size, _lib.current_stream(dev)),
                       "mg_maze_check_uniform_cell_size")
        if task_ids is None:
            task_ids = torch.arange(N, dtype=torch.int32) % T
        self.task_id = torch.as_tensor(task_ids, dtype=torch.int32).to(dev).contiguous()
        assert self.task_id.shape == (N,)
        # ---- per-env state --------------------------------------------------------------------
        self.grid = torch.zeros(2, N, dtype=torch.int32, device=dev)
        self.steps = torch.zeros(N, dtype=torch.int32, device=dev)
        self.ori_idx = torch.zeros(N, dtype=torch.int32, device=dev)
        self.ori = torch.zeros(N, dtype=torch.float64, device=dev)
        self.loc = torch.zeros(2, N, dtype=torch.float32, device=dev)
        self.life = torch.zeros(N, dtype=torch.float64, device=dev)
        st = _lib.MazeState()
        st.task_id, st.grid, st.steps = self.task_id.data_ptr(), self.grid.data_ptr(), self.steps.data_ptr()
        st.ori_idx, st.ori, st.loc, st.life = (self.ori_idx.data_ptr(), self.ori.data_ptr(), self.loc.data_ptr(),
                                               self.life.data_ptr())
        if self._tt == TASK_TYPES["SURVIVAL"]:
            # [N, nn] cells for the workgroup-per-env 3-D kernel; [max_food, N] food SLOTS for the lane-per-env 2-D kernel
            # (mg_maze_state.food_by_slot: lane e's k-th access is coalesced whatever task it runs)
            # (above the food-list bound the 2-D env keeps cells in the same lane-per-env order, [nn, N])
            shape = (self._max_food, N) if self._by_slot else ((nn, N) if self._BY_SLOT else (N, nn))
            self.cur_food = torch.zeros(*shape, dtype=torch.float64, device=dev)
            self.wait_refresh = torch.zeros(*shape, dtype=torch.uint8, device=dev)
            self.revival = torch.zeros(*shape, dtype=torch.int32, device=dev)
            st.cur_food, st.wait_refresh, st.revival = (self.cur_food.data_ptr(), self.wait_refresh.data_ptr(),
                                                        self.revival.data_ptr())
            st.food_env_stride, st.food_cell_stride = (1, N) if self._BY_SLOT else (nn, 1)
            st.food_by_slot = int(self._by_slot)
        self._state_c = st
        self._on_set_task()
        self.need_set_task = False
        self.need_reset = True

    def _check_table(self, n, min_cell_size):
        """Refuse a table this env cannot run, before set_task changes anything (a refused set_task leaves the env as it was)."""

    def _on_set_task(self):
        pass

    _BY_SLOT = False      # the class's SURVIVAL layout; _by_slot is the current table's (by cell above FOOD_LIST_MAX_CELLS)
    _by_slot = False
    _STATE_KEYS = ("grid", "steps", "ori_idx", "ori", "loc", "life", "cur_food", "wait_refresh", "revival")
    _FOOD_KEYS = ("cur_food", "wait_refresh", "revival")

    def _food_by_cell(self, key):
        """(slot layout) the [n*n, N] by-cell view of a SURVIVAL array — the checkpoint format, independent of how the kernel
        stores it: a listed cell's slot value, else what the cell holds for ever (its task's food value, wait 0, counter =
        its interval)."""
        tid = self.task_id.long()
        slot = self._cell_slot_t[tid].t().long()                                   # [nn, N]
        have = slot >= 0
        val = torch.gather(getattr(self, key), 0, slot.clamp(min=0))
        if key == "cur_food":
            rest = self._task_t["food_rewards"][tid].t()
        elif key == "revival":
            rest = self._task_t["food_interval"][tid].t()
        else:
            rest = torch.zeros_like(val)
        return torch.where(have, val, rest.to(val.dtype)).contiguous()

    def state_dict(self):
        """Per-env arrays + task_id: the SURVIVAL food arrays only make sense next to the task they were drawn for. The food
        arrays are always written by CELL ([n*n, N] for the 2-D env, [N, n*n] for the 3-D ones)."""
        sd = {}
        for k in self._STATE_KEYS:
            if hasattr(self, k):
                sd[k] = self._food_by_cell(k) if (self._by_slot and k in self._FOOD_KEYS) else getattr(self, k).clone()
        if hasattr(self, "task_id"):
            sd["task_id"] = self.task_id.clone()
        return sd

    def load_state_dict(self, sd):
        if "task_id" in sd and hasattr(self, "task_id"):          # first: the by-cell food arrays are read through the task's slots
            self.task_id.copy_(torch.as_tensor(sd["task_id"]).to(self.task_id.dtype))
        for k in self._STATE_KEYS:
            if hasattr(self, k) and k in sd:
                dst, src = getattr(self, k), torch.as_tensor(sd[k]).to(self.device)
                if self._by_slot and k in self._FOOD_KEYS:
                    if tuple(src.shape) != (self.n * self.n, self.num_envs):
                        raise ValueError("state_dict[%r] has shape %s, expected the by-cell view %s" % (k, tuple(src.shape), (self.n * self.n, self.num_envs)))
                    cells = self._food_cells_t[self.task_id.long()].t().long()   # [max_food, N]: the cell behind every slot
                    dst.copy_(torch.gather(src, 0, cells).to(dst.dtype))           # (slots past a task's n_food are never read)
                    continue
                if tuple(src.shape) != tuple(dst.shape):
                    raise ValueError("state_dict[%r] has shape %s, this env holds %s (same num_envs and maze size n needed)"
                                     % (k, tuple(src.shape), tuple(dst.shape)))
                dst.copy_(src.to(dst.dtype))
        if self._by_slot and hasattr(self, "revival") and all(k in sd for k in ("revival", "wait_refresh")):
            # the slot kernel never reads the counter of a slot that is not waiting (mg_maze_state.food_by_slot): a state with a
            # negative counter there cannot come out of reset() / step() — refuse it instead of diverging from maze_base.py:83-88
            if bool(((self.revival < 0) & (self.wait_refresh == 0)).any()):
                raise ValueError("state_dict: a food counter below zero on a cell that is not waiting (unreachable by reset / step)")

    # ------------------------------------------------------------------ episode control
    def reset(self, mask=None):
        if self.need_set_task:
            raise Exception("Must call \"set_task\" before reset")          # maze_env.py:49-50
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
            assert m.shape == (self.num_envs,)
        rc = self._lib.mg_maze_reset(self._tasks_c, self._tt, self.num_envs, self._state_c, _lib.ptr(m),
                                     _lib.current_stream(self.device))
        _lib.check(rc, "mg_maze_reset")
        self.need_reset = False
        return self._observe()

    def _check_step(self):
        if self.need_reset:
            raise Exception("Must \"reset\" before doing any actions")        # maze_env.py:60-61

    @property
    def reward64(self):
        return self._reward64

    def rollout(self, actions, obs_every=0):
        """`for t in range(T): step(actions[t])` without the host in the loop: same end state, rewards and dones bit for bit, for
        both task types and both settings of `auto_reset` (an env without it that is stepped past `done` goes on stepping, as
        in `step`). actions: [T, num_envs] ints (2-D, discrete 3-D) or float32 [T, num_envs, 2] (continuous 3-D), T >= 1.
        `obs_every` selects the steps that leave an observation (`rollout_obs_steps`): 0 = the last one only, k >= 1 = every
        k-th and the last. Returns (obs, reward, done, info): reward float32 [T, N] and done bool [T, N], fresh tensors per call
        (`self.rollout_reward64`: the exact float64 [T, N]); obs is the persistent [N, ...] buffer `step` returns when
        obs_every == 0, else a fresh [K, N, ...] tensor with one slice per recorded step (with auto_reset, the first
        observation of the next episode where that step ended one); info["steps"] the counters after the last step,
        info["obs_steps"] the K recorded step indices. The 2-D env runs ONE launch, the 3-D envs two per recorded step (the
        renderer only runs for those). Nothing synchronises: the call can be captured in a hipGraph like `step`. The
        persistent reward / done buffers of `step` are not written."""
        if self.need_set_task:
            raise Exception("Must call \"set_task\" before rollout")
        self._check_step()
        a = self._rollout_actions(actions)
        T = int(a.shape[0])
        idx = rollout_obs_steps(T, obs_every)
        N, dev = self.num_envs, self.device
        reward = torch.empty(T, N, dtype=torch.float32, device=dev)
        reward64 = torch.empty(T, N, dtype=torch.float64, device=dev)
        done = torch.empty(T, N, dtype=torch.bool, device=dev)
        obs = self._obs if int(obs_every) == 0 else torch.empty((len(idx),) + tuple(self._obs.shape), dtype=self._obs.dtype,
                                                                 device=dev)
        self._launch_rollout(a, T, int(obs_every), obs, reward, reward64, done)
        self.rollout_reward64 = reward64
        return obs, reward, done, {"steps": self.steps, "obs_steps": idx}

    def _rollout_actions(self, actions):
        """[T, N] int32 on the device; a wrong shape is a ValueError."""
        a = torch.as_tensor(actions, device=self.device)
        if a.dim() != 2 or a.shape[0] < 1 or a.shape[1] != self.num_envs:
            raise ValueError("rollout actions must be [T, num_envs = %d] ints in 0..3 with T >= 1, got %s"
                             % (self.num_envs, tuple(a.shape)))
        return a.to(torch.int32).contiguous()

    # ------------------------------------------------------------------ shortest-path fields and the expert
    _FIELD_KIND = None    # the class's own kind of field (metamaze/expert.py): MOVES_2D, TURNS or CELLS_3D
    _HAS_EXPERT = True

    def distance_field(self, sources=None, kind=None):
        """The shortest-path field of every task of the table, built on the GPU in one launch (mg_maze_distance_field, one
        workgroup per task; metamaze/expert.py defines the numbers): a `MazeDistanceField` whose `dist` int32 [T, K, n, n]
        holds the smallest number of env steps from each state onto a source cell, 0 on a source, -1 where none can be
        reached. `kind` defaults to the class's own (2-D: MOVES_2D, discrete 3-D: TURNS with K = 4 headings, continuous 3-D:
        CELLS_3D); `sources` is a bool / uint8 [T, n, n] mask, or None for each task's goal cell. The default goal field is
        built once per `set_task` and kept; every other call returns a fresh tensor. Nothing synchronises and a
        DeviceTaskTable never visits the host."""
        from . import expert as ex
        if self.need_set_task:
            raise Exception("Must call \"set_task\" before distance_field")
        kind = self._FIELD_KIND if kind is None else ex.check_kind(kind)
        n, T, dev = self.n, self._tasks_c.n_tasks, self.device
        default = sources is None and kind == self._FIELD_KIND
        if default and self._goal_field is not None:
            return self._goal_field
        src = None
        if sources is not None:
            src = torch.as_tensor(sources)
            if tuple(src.shape) != (T, n, n):
                raise ValueError("sources must be a [T = %d, n = %d, n] mask, got %s" % (T, n, tuple(src.shape)))
            if src.dtype not in (torch.bool, torch.uint8):
                raise ValueError("sources must be bool or uint8, got %s" % src.dtype)
            src = src.to(dev).to(torch.uint8).contiguous()
        dist = torch.empty(T, ex.orientations(kind), n, n, dtype=torch.int32, device=dev)
        rc = self._lib.mg_maze_distance_field(self._tasks_c, kind, _lib.ptr(src), _lib.ptr(dist), _lib.current_stream(dev))
        _lib.check(rc, "mg_maze_distance_field")
        field = ex.MazeDistanceField(dist, kind, n)
        if default:
            self._goal_field = field
        return field

    def _expert_field(self, field, what):
        """The field an expert call runs on, checked: None = the cached goal field; else one of this env's own kind, n, T and
        device. Raises before anything is written."""
        from . import expert as ex
        if self.need_set_task:
            raise Exception("Must call \"set_task\" before %s" % what)
        self._check_step()
        if field is None:
            return self.distance_field()
        if not isinstance(field, ex.MazeDistanceField):
            raise TypeError("field must be a MazeDistanceField, got %s" % type(field).__name__)
        if field.kind != self._FIELD_KIND:
            raise ValueError("%s needs a %s field, got %s" % (what, ex.KIND_NAMES[self._FIELD_KIND], ex.KIND_NAMES[field.kind]))
        if field.n != self.n or field.num_tasks != self._tasks_c.n_tasks:
            raise ValueError("the field is for T = %d tasks of n = %d, the env holds T = %d of n = %d"
                             % (field.num_tasks, field.n, self._tasks_c.n_tasks, self.n))
        d = field.device
        if not (d.type == self.device.type and (d.index or 0) == (self.device.index or 0)):
            raise ValueError("the field lives on %s, the env on %s" % (d, self.device))
        return field

    def expert_action(self, field=None):
        """The expert's action for every env, int32 [N], one launch (mg_maze_expert_action): the lowest action whose successor
        under the step's own rule is one step nearer in `field` (a `MazeDistanceField` of the class's own kind; None = the
        cached goal field), 0 where there is none (on a source, in an unreachable state). Reads the envs' cells, headings and
        task ids and writes a persistent buffer, overwritten by the next call; nothing synchronises, so
        `env.step(env.expert_action())` can be captured in a hipGraph. The continuous maze has no expert of this kind and
        raises NotImplementedError; its expert steers, see `MetaMazeContinuous3D.steer_action`."""
        if not self._HAS_EXPERT:
            raise NotImplementedError("the continuous maze has no expert (distance_field gives its cell-level field)")
        field = self._expert_field(field, "expert_action")
        if self._expert_action is None:
            self._expert_action = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        rc = self._lib.mg_maze_expert_action(self._tasks_c, field.kind, _lib.ptr(field.dist), self.num_envs, self._state_c,
                                             _lib.ptr(self._expert_action), _lib.current_stream(self.device))
        _lib.check(rc, "mg_maze_expert_action")
        return self._expert_action

    def render(self, mode="human"):
        raise NotImplementedError("rendering is out of scope for the batched engine")

    def close(self):
        pass


class MetaMaze2D(_MazeBatch):
    """maze_env.py:155-212. obs float32 [N, 2v+1, 2v+1]; action int in {0..3} per env."""
    _BY_SLOT = True       # SURVIVAL arrays per food slot, [max_food, N] (mg_maze_state.food_by_slot)
    _FIELD_KIND = 0       # expert.MOVES_2D

    def __init__(self, num_envs=1, device="cuda", enable_render=False, render_scale=480, max_steps=5000,
                 task_type="SURVIVAL", view_grid=2, auto_reset=False):
        super().__init__(num_envs, device, max_steps, task_type, auto_reset)
        self.view_grid = int(view_grid)
        self.action_space = Discrete(4)
        w = 2 * self.view_grid + 1
        self.observation_space = Box(low=-1.0, high=2.0, shape=(w, w), dtype=np.float32)
        self._obs = torch.zeros(self.num_envs, w, w, dtype=torch.float32, device=self.device)

    def _launch(self, action):
        rc = self._lib.mg_maze2d_step(self._tasks_c, self._tt, self.max_steps, self.view_grid, int(self.auto_reset),
                                      self.num_envs, self._state_c, _lib.ptr(action), _lib.ptr(self._obs),
                                      _lib.ptr(self._reward), _lib.ptr(self._reward64), _lib.ptr(self._done),
                                      _lib.current_stream(self.device))
        _lib.check(rc, "mg_maze2d_step")

    def _observe(self):
        self._launch(None)
        return self._obs

    def step(self, action):
        self._check_step()
        a = torch.as_tensor(action, device=self.device).to(torch.int32).contiguous()
        assert a.shape == (self.num_envs,), "action must be [num_envs] ints in 0..3"
        self._launch(a)
        return self._obs, self._reward, self._done, {"steps": self.steps}

    def _launch_rollout(self, a, T, obs_every, obs, reward, reward64, done):
        rc = self._lib.mg_maze2d_rollout(self._tasks_c, self._tt, self.max_steps, self.view_grid, int(self.auto_reset),
                                         self.num_envs, self._state_c, T, obs_every, _lib.ptr(a), _lib.ptr(obs),
                                         _lib.ptr(reward), _lib.ptr(reward64), _lib.ptr(done),
                                         _lib.current_stream(self.device))
        _lib.check(rc, "mg_maze2d_rollout")

    def rollout_policy(self, policy, steps, policy_ids=None, state=None, seed=0, record=False, obs_every=0, episodic=False):
        """`steps` closed-loop env steps in ONE launch: env e evaluates policy `policy_ids[e]` of `policy` (a `MazePolicy`;
        `policy_ids=None` = e % P) on its own window, previous action, reward and done inside the kernel and steps with the
        result (metamaze/policy.py defines the arithmetic exactly). `state` is the carry of the previous call (a
        `MazePolicyState`; None = a fresh one); it is not written, the end carry comes back as `.state` of the result with
        `step` advanced by `steps`. `seed` keys the exploration draws of a policy with epsilon and the sampling draws of a
        policy with a temperature (which goes through mg_maze2d_policy_rollout_sampled; everything else here is the same).
        With `auto_reset` the policy's
        memory survives a done (the step after it sees the next episode's first window, prev_done = 1 and the ending step's
        reward and action); `episodic=True` clears the carry at a done instead. Returns a `MazePolicyRollout`: ret_total,
        ret_episode, episode_len, episodes and state always; actions, reward, reward64, done [steps, N] when `record=True`,
        else None (the launch then writes nothing per step). `obs_every` >= 1 keeps a fresh [K, N, w, w] tensor of the
        observations `rollout_obs_steps` selects; 0 keeps the last one only, in the persistent buffer `step` returns, which
        is written either way. Nothing synchronises when `policy_ids` is None, a host array, or the device tensor of the
        previous call (the same object, unchanged; any other device tensor is read back once to validate it). A refused
        call (an id out of range, a policy built for another view_grid, a carry of another N or H, steps < 1) raises and
        leaves the env and the carry as they were."""
        from .policy import MazePolicy, MazePolicyState
        if self.need_set_task:
            raise Exception("Must call \"set_task\" before rollout_policy")
        self._check_step()
        if not isinstance(policy, MazePolicy):
            raise TypeError("policy must be a MazePolicy, got %s" % type(policy).__name__)
        T, N, dev, P, H = int(steps), self.num_envs, self.device, policy.num_policies, policy.hidden
        if T < 1:
            raise ValueError("steps must be at least 1, got %d" % T)
        idx = rollout_obs_steps(T, obs_every)
        if policy.view_grid != self.view_grid:
            raise ValueError("the policy was built for view_grid = %d, the env has %d" % (policy.view_grid, self.view_grid))
        state, seed = _policy.check_discrete_carry(state, MazePolicyState, N, H, T, seed, dev)
        ids_d = _policy.policy_ids(self, policy_ids, P)
        params, thr = policy.to(dev)
        inv_t = policy.inv_temperature_on(dev)
        # everything is checked: from here on the env and the new carry are written
        carry = MazePolicyState(*[v.to(dev).clone().contiguous() for v in (state.h, state.prev_action, state.prev_reward,
                                                                           state.prev_done)], step=state.step + T)
        desc = _lib.MazePolicyDesc(P, H, policy.view_grid, params.data_ptr(), thr.data_ptr() if thr is not None else None)
        carry_c = _lib.MazePolicyCarry(carry.h.data_ptr(), carry.prev_action.data_ptr(), carry.prev_reward.data_ptr(),
                                       carry.prev_done.data_ptr())
        res = self._rollout_results(T, idx, obs_every, record, carry)
        obs = res.obs
        head = (self._tasks_c, self._tt, self.max_steps, self.view_grid, int(self.auto_reset), N, self._state_c, T, int(obs_every),
                desc, _lib.ptr(ids_d), carry_c)
        tail = (seed, state.step, int(bool(episodic)), _lib.ptr(self._obs), _lib.ptr(res.ret_total), _lib.ptr(res.ret_episode),
                _lib.ptr(res.episode_len), _lib.ptr(res.episodes), _lib.ptr(res.actions), _lib.ptr(res.reward),
                _lib.ptr(res.reward64), _lib.ptr(res.done), _lib.ptr(obs) if int(obs_every) > 0 else None,
                _lib.current_stream(dev))
        if inv_t is None:
            _lib.check(self._lib.mg_maze2d_policy_rollout(*(head + tail)), "mg_maze2d_policy_rollout")
        else:
            _lib.check(self._lib.mg_maze2d_policy_rollout_sampled(*(head + (_lib.ptr(inv_t),) + tail)),
                       "mg_maze2d_policy_rollout_sampled")
        return res

    def rollout_expert(self, steps, field=None, record=False, obs_every=0):
        """`steps` closed-loop env steps in ONE launch (mg_maze2d_expert_rollout): before every step each env takes
        `expert_action` on the state it holds (after an auto-reset: the new episode's start) and steps with it. `field` is a
        MOVES_2D `MazeDistanceField` (None = the cached goal field, the shortest path in ESCAPE; in SURVIVAL the expert
        simply descends the field it is given). Returns a `MazePolicyRollout` as `rollout_policy` does, with `state=None`:
        ret_total, ret_episode, episode_len, episodes always; actions, reward, reward64, done [steps, N] when `record=True`,
        else None (the launch then writes nothing per step); `obs_every` as for `rollout_policy`. Replaying the recorded
        actions through `rollout` gives the same records and end state bit for bit. Nothing synchronises. A refused call (a
        field of another n, T, kind or device, steps < 1, a call before set_task or reset) raises and leaves the env and the
        field as they were."""
        T, N, dev = int(steps), self.num_envs, self.device
        if self.need_set_task:
            raise Exception("Must call \"set_task\" before rollout_expert")
        self._check_step()
        if T < 1:
            raise ValueError("steps must be at least 1, got %d" % T)
        idx = rollout_obs_steps(T, obs_every)
        field = self._expert_field(field, "rollout_expert")
        res = self._rollout_results(T, idx, obs_every, record, None)
        obs = res.obs
        rc = self._lib.mg_maze2d_expert_rollout(self._tasks_c, self._tt, self.max_steps, self.view_grid, int(self.auto_reset), N,
                                                self._state_c, T, int(obs_every), _lib.ptr(field.dist), _lib.ptr(self._obs),
                                                _lib.ptr(res.ret_total), _lib.ptr(res.ret_episode), _lib.ptr(res.episode_len),
                                                _lib.ptr(res.episodes), _lib.ptr(res.actions), _lib.ptr(res.reward),
                                                _lib.ptr(res.reward64), _lib.ptr(res.done),
                                                _lib.ptr(obs) if int(obs_every) > 0 else None, _lib.current_stream(dev))
        _lib.check(rc, "mg_maze2d_expert_rollout")
        return res

    def _rollout_results(self, T, idx, obs_every, record, carry):
        """The `MazePolicyRollout` of a T-step launch, its tensors allocated: the four results always, the observations kept
        (`obs_every` = 0: the persistent buffer), the four [T, N] records with `record`, else None. `rollout_policy` and
        `rollout_expert` share it."""
        from .policy import MazePolicyRollout
        N, dev = self.num_envs, self.device
        obs = self._obs if int(obs_every) == 0 else torch.empty((len(idx),) + tuple(self._obs.shape), dtype=torch.float32, device=dev)
        res = MazePolicyRollout(torch.empty(N, dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.float64, device=dev),
                                torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev),
                                carry, obs, idx)
        if record:
            res.actions = torch.empty(T, N, dtype=torch.int32, device=dev)
            res.reward = torch.empty(T, N, dtype=torch.float32, device=dev)
            res.reward64 = torch.empty(T, N, dtype=torch.float64, device=dev)
            res.done = torch.empty(T, N, dtype=torch.bool, device=dev)
        return res


class _Maze3D(_MazeBatch):
    def __init__(self, num_envs, device, resolution, max_steps, task_type, auto_reset, collision_dist=0.20,
                 max_vision_range=12.0, fol_angle=0.6 * PI, obs_dtype=torch.int32):
        super().__init__(num_envs, device, max_steps, task_type, auto_reset)
        self.resolution_horizon, self.resolution_vertical = int(resolution[0]), int(resolution[1])
        self.collision_dist, self.max_vision_range, self.fol_angle = collision_dist, max_vision_range, fol_angle
        H, V = self.resolution_horizon, self.resolution_vertical
        self.observation_space = Box(low=np.zeros((H, V, 3), np.float32), high=np.full((H, V, 3), 256, np.float32),
                                     dtype=np.float32)      # declared like the reference (maze_env.py:38-40)
        # int32 is the reference's frame dtype (values exceed 255: ray_caster_utils.py light > 1);
        # torch.uint8 selects the saturating fast path (not reference-exact where the reference exceeds 255)
        assert obs_dtype in (torch.int32, torch.uint8)
        self.obs_dtype = obs_dtype
        self._obs = torch.zeros(self.num_envs, H, V, 3, dtype=obs_dtype, device=self.device)
        self._tex_version = None

    def __getattr__(self, name):
        # `env.rollout_policy` of a 3-D env is looked up here, on the env, and the 3-D classes carry no attribute of that
        # name: the 2-D policy tests pin that `rollout_policy`, which there takes a `MazePolicy` on the window, is an attribute
        # of the 2-D class alone (tests/test_maze_policy.py, tests/test_maze_policy_gpu.py: hasattr on the 3-D classes is
        # False). The method itself, with its documentation, is `_rollout_policy_3d` of the env's class. No bound method is
        # kept on the env, so the env stays free of reference cycles.
        if name == "rollout_policy":
            return self._rollout_policy_3d
        raise AttributeError("%r object has no attribute %r" % (type(self).__name__, name))

    def _max_ray_records(self, min_cell_size):
        return 2 * int(self.max_vision_range / min_cell_size) + 5

    def _check_table(self, n, min_cell_size):
        # the renderer keeps at most 127 translucent cells per ray and mg_maze3d_step refuses a larger bound; said here, before
        # set_task replaces the table — a view built for the previous table must never meet this one
        bound = min(2 * n + 1, self._max_ray_records(min_cell_size))
        if bound > MAX_RAY_RECORDS:
            raise ValueError("maze n=%d with cell size %.17g at max_vision_range %g: a ray may cross %d translucent cells, the "
                             "renderer keeps at most %d (n <= 63, or every cell size above max_vision_range / %d)"
                             % (n, min_cell_size, self.max_vision_range, bound, MAX_RAY_RECORDS, (MAX_RAY_RECORDS - 5) // 2 + 1))

    def _on_set_task(self):
        self._build_view()

    def _build_view(self):
        lib, dev = self._lib, self.device
        H, V = self.resolution_horizon, self.resolution_vertical
        v = _lib.MazeView()
        v.res_h, v.res_v = H, V
        v.max_vision, v.l_focal, v.text_size = self.max_vision_range, 0.20, 1.0     # maze_discrete_3d.py:113-117
        v.tan_half_fov = float(np.tan(self.fol_angle / 2))                           # ray_caster_utils.py:68
        v.collision_dist = self.collision_dist
        cc, cs = np.zeros(H, np.float64), np.zeros(H, np.float64)
        _lib.check(lib.mg_maze_view_tables(H, v.tan_half_fov, v.l_focal, cc.ctypes.data, cs.ctypes.data),
                   "mg_maze_view_tables")
        self._col_cos, self._col_sin = torch.from_numpy(cc).to(dev), torch.from_numpy(cs).to(dev)
        v.col_cos, v.col_sin = self._col_cos.data_ptr(), self._col_sin.data_ptr()
        ori = np.asarray([0.0, 0.5, 1.0, 1.5], dtype="float32") * PI                 # maze_discrete_3d.py:46
        s4, c4 = np.sin(ori).astype(np.float32), np.cos(ori).astype(np.float32)
        for i in range(4):
            v.ori_sin[i], v.ori_cos[i] = float(s4[i]), float(c4[i])
        tex, ceil = MAZE_TASK_MANAGER.packed_textures()
        self._tex_t = torch.from_numpy(tex.view(np.int32).copy()).to(dev).contiguous()   # uint32 bits
        self._ceil_t = torch.from_numpy(ceil.view(np.int32).copy()).to(dev).contiguous()
        v.textures, v.ceil_texture = self._tex_t.data_ptr(), self._ceil_t.data_ptr()
        v.n_textures, v.tex_size = tex.shape[0], tex.shape[1]
        v.obs_format = 1 if self.obs_dtype == torch.uint8 else 0
        # DDA_2D (ray_caster_utils.py:31) stops once hit_dist >= max_vision: a ray crosses at most
        # floor(max_vision / cell_size) + 1 cell boundaries per axis plus the final overshoot, so it can
        # record at most 2*floor(mv/cs) + 4 translucent cells (incl. the start cell) whatever n is
        v.max_ray_records = self._max_ray_records(self._min_cell_size)
        v.uniform_cell_size = self._uniform_cell_size
        self._view_c = v
        self._tex_version = MAZE_TASK_MANAGER.version

    def _launch(self, action, continuous):
        if self._tex_version != MAZE_TASK_MANAGER.version:
            self._build_view()
        rc = self._lib.mg_maze3d_step(self._tasks_c, self._view_c, self._tt, self.max_steps, int(continuous),
                                      int(self.auto_reset), self.num_envs, self._state_c, _lib.ptr(action),
                                      _lib.ptr(self._obs), _lib.ptr(self._reward), _lib.ptr(self._reward64),
                                      _lib.ptr(self._done), _lib.current_stream(self.device))
        _lib.check(rc, "mg_maze3d_step")

    _CONTINUOUS = False

    def _launch_rollout(self, a, T, obs_every, obs, reward, reward64, done):
        if self._tex_version != MAZE_TASK_MANAGER.version:
            self._build_view()
        rc = self._lib.mg_maze3d_rollout(self._tasks_c, self._view_c, self._tt, self.max_steps, int(self._CONTINUOUS),
                                         int(self.auto_reset), self.num_envs, self._state_c, T, obs_every, _lib.ptr(a),
                                         _lib.ptr(obs), _lib.ptr(reward), _lib.ptr(reward64), _lib.ptr(done),
                                         _lib.current_stream(self.device))
        _lib.check(rc, "mg_maze3d_rollout")

    def demonstrate(self, steps, field=None, record=False, obs_every=0):
        """`steps` closed-loop env steps with the expert inside the launches (mg_maze3d_expert_rollout): before every step each
        env takes its expert's action on the state it holds (after an auto-reset: the new episode's start) and steps with
        it. The discrete env uses `expert_action`'s rule on a TURNS field, the continuous env `steer_action`'s rule on a
        CELLS_3D field; `field` is a `MazeDistanceField` of that kind (None = the cached goal field, the way out in ESCAPE; in
        SURVIVAL the expert simply descends the field it is given). Returns a `MazePolicyRollout` as
        `MetaMaze2D.rollout_expert` does, with `state=None`: ret_total, ret_episode, episode_len, episodes always; actions
        (int32 [steps, N], continuous: float32 [steps, N, 2]), reward, reward64, done [steps, N] when `record=True`, else None
        (the launches then write nothing per step). obs and obs_steps as in `rollout`: obs_every == 0 keeps the last frame
        only, in the persistent buffer `step` returns; k >= 1 returns a fresh [K, N, H, V, 3] tensor in the env's obs_dtype
        with the frames `rollout_obs_steps` selects. Two launches per recorded frame, as `rollout`: the steps up to it
        without a picture, then the renderer. Replaying the recorded actions through `rollout` gives the same records,
        frames and end state bit for bit. Nothing synchronises. A refused call (a field of another n, T, kind or device,
        steps < 1, obs_every < 0, a call before set_task or reset) raises before anything is written."""
        from .policy import MazePolicyRollout
        T, N, dev = int(steps), self.num_envs, self.device
        if self.need_set_task:
            raise Exception("Must call \"set_task\" before demonstrate")
        self._check_step()
        if T < 1:
            raise ValueError("steps must be at least 1, got %d" % T)
        idx = rollout_obs_steps(T, obs_every)
        field = self._expert_field(field, "demonstrate")
        if self._tex_version != MAZE_TASK_MANAGER.version:
            self._build_view()
        obs = self._obs if int(obs_every) == 0 else torch.empty((len(idx),) + tuple(self._obs.shape), dtype=self._obs.dtype,
                                                                 device=dev)
        res = MazePolicyRollout(torch.empty(N, dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.float64, device=dev),
                                torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev),
                                None, obs, idx)
        if record:
            res.actions = (torch.empty(T, N, 2, dtype=torch.float32, device=dev) if self._CONTINUOUS
                           else torch.empty(T, N, dtype=torch.int32, device=dev))
            res.reward = torch.empty(T, N, dtype=torch.float32, device=dev)
            res.reward64 = torch.empty(T, N, dtype=torch.float64, device=dev)
            res.done = torch.empty(T, N, dtype=torch.bool, device=dev)
        rc = self._lib.mg_maze3d_expert_rollout(self._tasks_c, self._view_c, self._tt, self.max_steps, int(self._CONTINUOUS),
                                                int(self.auto_reset), N, self._state_c, T, int(obs_every), _lib.ptr(field.dist),
                                                _lib.ptr(obs), _lib.ptr(res.ret_total), _lib.ptr(res.ret_episode),
                                                _lib.ptr(res.episode_len), _lib.ptr(res.episodes), _lib.ptr(res.actions),
                                                _lib.ptr(res.reward), _lib.ptr(res.reward64), _lib.ptr(res.done),
                                                _lib.current_stream(dev))
        _lib.check(rc, "mg_maze3d_expert_rollout")
        return res

    _pooled = None

    def pooled_observation(self, grid):
        """The persistent frame buffer pooled over `grid` = (Gh, Gv), float32 [N, Gh, Gv, 3], one launch
        (mg_maze3d_pool_features): the features a `Maze3DPolicy` reads (metamaze/policy.py `pool_reference` is the
        definition, reproduced bit for bit), a cheap low-resolution observation for a policy kept in torch. The grid sides
        are in [1, 16] and must divide the resolution. The output is a persistent buffer per grid, overwritten by the next
        call with that grid; nothing synchronises, so `step` followed by `pooled_observation` can be captured in a hipGraph."""
        from . import policy as mp
        bh, bv = mp.check_grid_divides(grid, (self.resolution_horizon, self.resolution_vertical))
        gh, gv = mp.check_grid(grid)
        if self.need_set_task:
            raise Exception("Must call \"set_task\" before pooled_observation")
        if self._pooled is None:
            self._pooled = {}
        if (gh, gv) not in self._pooled:
            self._pooled[(gh, gv)] = torch.zeros(self.num_envs, gh, gv, 3, dtype=torch.float32, device=self.device)
        out = self._pooled[(gh, gv)]
        rc = self._lib.mg_maze3d_pool_features(self._view_c, self.num_envs, _lib.ptr(self._obs), gh, gv, float(mp.pool_scale(bh, bv)),
                                               _lib.ptr(out), _lib.current_stream(self.device))
        _lib.check(rc, "mg_maze3d_pool_features")
        return out

    def _rollout_policy(self, policy, steps, policy_ids, state, seed, record, obs_every, episodic):
        """`rollout_policy` of the two 3-D envs. Everything is checked before anything is written."""
        from . import policy as mp
        cls = mp.Maze3DSteerPolicy if self._CONTINUOUS else mp.Maze3DPolicy
        if self.need_set_task:
            raise Exception("Must call \"set_task\" before rollout_policy")
        self._check_step()
        if not isinstance(policy, cls):
            raise TypeError("policy must be a %s, got %s" % (cls.__name__, type(policy).__name__))
        T, N, dev, P, H = int(steps), self.num_envs, self.device, policy.num_policies, policy.hidden
        if T < 1:
            raise ValueError("steps must be at least 1, got %d" % T)
        idx = rollout_obs_steps(T, obs_every)
        bh, bv = mp.check_grid_divides(policy.grid, (self.resolution_horizon, self.resolution_vertical))
        if self._CONTINUOUS:
            if state is None:
                state = mp.Maze3DPolicyState(N, H, dev)
            else:
                _policy.check_continuous_carry(state, mp.Maze3DPolicyState, N, H, 2, dev, "Maze3DPolicyState(N, H, device)",
                                               "num_envs=%d, hidden=%d" % (N, H))
            step0 = 0
        else:
            state, seed = _policy.check_discrete_carry(state, mp.MazePolicyState, N, H, T, seed, dev)
            step0 = state.step
        ids_d = _policy.policy_ids(self, policy_ids, P)
        up = policy.to(dev)
        params, thr = (up, None) if self._CONTINUOUS else up
        if self._tex_version != MAZE_TASK_MANAGER.version:
            self._build_view()
        # everything is checked: from here on the env, the frame buffer and the new carry are written
        fields = [v.to(dev).clone().contiguous() for v in (state.h, state.prev_action, state.prev_reward, state.prev_done)]
        carry = mp.Maze3DPolicyState.of(*fields) if self._CONTINUOUS else mp.MazePolicyState(*fields, step=state.step + T)
        desc = _lib.Maze3DPolicyDesc(P, H, policy.grid[0], policy.grid[1], int(self._CONTINUOUS), float(mp.pool_scale(bh, bv)),
                                     params.data_ptr(), thr.data_ptr() if thr is not None else None)
        carry_c = _lib.MazePolicyCarry(carry.h.data_ptr(), carry.prev_action.data_ptr(), carry.prev_reward.data_ptr(),
                                       carry.prev_done.data_ptr())
        obs = self._obs if int(obs_every) == 0 else torch.empty((len(idx),) + tuple(self._obs.shape), dtype=self._obs.dtype,
                                                                 device=dev)
        res = mp.MazePolicyRollout(torch.empty(N, dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.float64, device=dev),
                                   torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev),
                                   carry, obs, idx)
        if record:
            res.actions = (torch.empty(T, N, 2, dtype=torch.float32, device=dev) if self._CONTINUOUS
                           else torch.empty(T, N, dtype=torch.int32, device=dev))
            res.reward = torch.empty(T, N, dtype=torch.float32, device=dev)
            res.reward64 = torch.empty(T, N, dtype=torch.float64, device=dev)
            res.done = torch.empty(T, N, dtype=torch.bool, device=dev)
        rc = self._lib.mg_maze3d_policy_rollout(self._tasks_c, self._view_c, self._tt, self.max_steps, int(self._CONTINUOUS),
                                                int(self.auto_reset), N, self._state_c, T, int(obs_every), desc, _lib.ptr(ids_d),
                                                carry_c, seed, step0, int(bool(episodic)), _lib.ptr(self._obs),
                                                _lib.ptr(obs) if int(obs_every) > 0 else None, _lib.ptr(res.ret_total),
                                                _lib.ptr(res.ret_episode), _lib.ptr(res.episode_len), _lib.ptr(res.episodes),
                                                _lib.ptr(res.actions), _lib.ptr(res.reward), _lib.ptr(res.reward64),
                                                _lib.ptr(res.done), _lib.current_stream(dev))
        _lib.check(rc, "mg_maze3d_policy_rollout")
        return res


class MetaMazeDiscrete3D(_Maze3D):
    """maze_env.py:16-83. action int in {0..3}: turn left / right, step back / forward."""

    def __init__(self, num_envs=1, device="cuda", enable_render=False, render_scale=480, resolution=(320, 320),
                 max_steps=5000, task_type="SURVIVAL", auto_reset=False, obs_dtype=torch.int32):
        super().__init__(num_envs, device, resolution, max_steps, task_type, auto_reset, obs_dtype=obs_dtype)
        self.action_space = Discrete(4)

    _FIELD_KIND = 2       # expert.TURNS

    def _rollout_policy_3d(self, policy, steps, policy_ids=None, state=None, seed=0, record=False, obs_every=0, episodic=False):
        """`steps` closed-loop env steps with the controller inside the launches (mg_maze3d_policy_rollout): env e pools the
        frame of the state it holds over the policy's grid, evaluates policy `policy_ids[e]` of `policy` (a `Maze3DPolicy`;
        None = e % P) on the features, its previous action, reward and done, and steps with the result (metamaze/policy.py
        defines the arithmetic exactly; `Maze3DPolicy.reference` is the oracle). One render of the current state first (so
        the call is right after `load_state_dict`, whatever the frame buffer holds), then one advance launch and one render
        per step. `state` is the carry of the previous call (a `MazePolicyState`; None = a fresh one); it is not written, the
        end carry comes back as `.state` with `step` advanced by `steps`. `seed` keys the exploration draws of a policy with
        epsilon. With `auto_reset` the memory survives a done; `episodic=True` clears the carry at a done instead. Returns a
        `MazePolicyRollout` as `MetaMaze2D.rollout_policy` does: ret_total, ret_episode, episode_len, episodes and state
        always; actions int32, reward, reward64, done [steps, N] when `record=True`, else None; obs and obs_steps as in
        `demonstrate` (obs_every == 0: the persistent buffer with the last frame; k >= 1: a fresh [K, N, H, V, 3] tensor, the
        persistent buffer then holds the last frame that was not kept). Replaying the recorded actions through `rollout`
        gives the same records, frames and end state bit for bit. Nothing synchronises (`policy_ids` as for
        `MetaMaze2D.rollout_policy`). A refused call (another policy class, a grid that does not divide the resolution, a
        carry of another N or H, an id out of range, steps < 1, obs_every < 0, a call before set_task or reset) raises and
        leaves the env, the carry and the frame buffer as they were."""
        return self._rollout_policy(policy, steps, policy_ids, state, seed, record, obs_every, episodic)

    def _observe(self):
        self._launch(None, False)
        return self._obs

    def step(self, action):
        self._check_step()
        a = torch.as_tensor(action, device=self.device).to(torch.int32).contiguous()
        assert a.shape == (self.num_envs,), "action must be [num_envs] ints in 0..3"
        self._launch(a, False)
        return self._obs, self._reward, self._done, {"steps": self.steps}


class MetaMazeContinuous3D(_Maze3D):
    """maze_env.py:85-153. action float32 [N,2] = (turn rate, walk speed), each clipped to [-1,1]."""

    def __init__(self, num_envs=1, device="cuda", enable_render=False, render_scale=480, resolution=(320, 320),
                 max_steps=5000, task_type="SURVIVAL", auto_reset=False, obs_dtype=torch.int32):
        super().__init__(num_envs, device, resolution, max_steps, task_type, auto_reset, obs_dtype=obs_dtype)
        self.action_space = Box(low=np.array([-1.0, -1.0]), high=np.array([1.0, 1.0]), dtype=np.float32)

    _CONTINUOUS = True
    _FIELD_KIND = 1       # expert.CELLS_3D
    _HAS_EXPERT = False
    _steer_action = None

    def _rollout_actions(self, actions):
        a = torch.as_tensor(actions, dtype=torch.float32, device=self.device)
        if a.dim() != 3 or a.shape[0] < 1 or tuple(a.shape[1:]) != (self.num_envs, 2):
            raise ValueError("rollout actions must be float32 [T, num_envs = %d, 2] with T >= 1, got %s"
                             % (self.num_envs, tuple(a.shape)))
        return a.contiguous()

    def _rollout_policy_3d(self, policy, steps, policy_ids=None, state=None, record=False, obs_every=0, episodic=False):
        """`env.rollout_policy` of the discrete 3-D maze (`MetaMazeDiscrete3D._rollout_policy_3d`) for the continuous maze: `policy` is a `Maze3DSteerPolicy`, whose two outputs,
        NaN -> 0 and clamped to [-1, 1], are (turn, walk): that value is stepped with, recorded (actions float32
        [steps, N, 2]) and fed back as the previous action. No exploration, so no seed. `state` is a `Maze3DPolicyState`
        (None = a fresh one); it is not written, the end carry comes back as `.state`."""
        return self._rollout_policy(policy, steps, policy_ids, state, 0, record, obs_every, episodic)

    def _observe(self):
        self._launch(None, True)
        return self._obs

    def steer_action(self, field=None):
        """The steering expert's action for every env, float32 [N, 2] = (turn, walk), one launch (mg_maze_steer_action): towards
        the centre of the first neighbour cell one step nearer in `field` (a CELLS_3D `MazeDistanceField`; None = the cached
        goal field) — walk when the heading is within 9 degrees of it, else turn towards it; (0, 0) on a source, in an
        unreachable cell or off the grid. metamaze/expert.py `steer_action_reference` is the definition, reproduced bit for
        bit. Reads the envs' cells, locations, headings and task ids and writes a persistent buffer, overwritten by the next
        call; nothing synchronises, so `env.step(env.steer_action())` can be captured in a hipGraph."""
        field = self._expert_field(field, "steer_action")
        if self._steer_action is None:
            self._steer_action = torch.zeros(self.num_envs, 2, dtype=torch.float32, device=self.device)
        rc = self._lib.mg_maze_steer_action(self._tasks_c, _lib.ptr(field.dist), self.num_envs, self._state_c,
                                            _lib.ptr(self._steer_action), _lib.current_stream(self.device))
        _lib.check(rc, "mg_maze_steer_action")
        return self._steer_action

    def step(self, action):
        self._check_step()
        a = torch.as_tensor(action, dtype=torch.float32, device=self.device).contiguous()
        assert a.shape == (self.num_envs, 2), "action must be [num_envs, 2]"
        self._launch(a, True)
        return self._obs, self._reward, self._done, {"steps": self.steps}
