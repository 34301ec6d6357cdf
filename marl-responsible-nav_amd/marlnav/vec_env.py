"""VecGridEnv: E independent CustomMAEnv episodes resident on one MI355X.

Tensor API over libgridenv (include/gridenv.h).  One ``step`` is the reference's
``CustomMAEnv.step`` (custom/ma_customenv.py:217-334) applied to all E envs at once, plus the
per-step reward/score arithmetic of ``MADDPGAgent.train`` (maddpg/agent.py:124-173) and an
optional auto-reset (the ``break`` + ``env.reset()`` of maddpg/agent.py:241 / main_custom.py:129).

Layouts (device tensors, owned by the env and overwritten by the next call):
  obs        [K, E, H, W] float32   agent-major: obs[k] is RL agent k's actor input batch
             (obs_dtype=torch.bfloat16: the same values, exact, in half the bytes)
  reward, fear, shaped      [E, K] float64
  term, trunc               [E, K] uint8;  done [E] uint8
  mask       [E, K] int16 (9-bit action mask, bit a = action a allowed)
  crashes, apples, ep_len   [E] int32;  ep_return, ep_fear [E] float64
  debug outputs (debug=True): actions/mdr/final_pos [E, N] int32, crash_bits/restr_bits [E] uint8
  stats (stats=True): [rows, 8] float64 per-block partial sums of the step (_lib.STATS_NAMES)
  fear_row (fear_rows=True): [E, K, N] float64, Resp[k][j] of FeAR_4_one_actor(actor = k): how much RL
             agent k restricted agent j this step (its np.sum is fear[e, k]; zeros with FeAR off)
  fear_alt (fear_alt=True): [E, K, 9] float64, the step's FeAR of RL agent k had it played action a while
             everybody else did what they did (gw_set_fear_alt): fear_alt[e, k, actions[e, k]] is
             fear[e, k] and fear_alt[e, k, mdr[e, k]] is 0.0, bit for bit; zeros with FeAR off
  feal (feal=True): [E, N] float64, Responsibility.FeAL of every world agent on the step's pre-move
             world (gw_set_feal): how much of agent i's action space survived what the others did,
             against what would have survived had they played their moves de rigueur
  feal_valid (feal=True): [E, N, 2] int16 (views of the u16 bit sets, as mask): bit b of [..., 0] /
             [..., 1] = action b of agent i is valid while the others play their MdR / their actual
             actions; feal = clip(popcount([..., 1]) / (popcount([..., 0]) + 1e-6), -1, 1).
             Needs fear=True (fear_weight=0.0 keeps shaped == reward)
  resp_full (fear_full=True): [E, N, N] float64, Responsibility.FeAR of the step's pre-move world with
             every world agent as actor and every agent listed (gw_set_fear_full): resp_full[e, i, j] is
             how much actor i (RL or scripted) restricted agent j; the diagonal is 0.0
  resp_valid (fear_full=True): [E, N, N, 2] int16 (views of the u16 bit sets): bit b of [..., i, j, 1] =
             action b of agent j is valid with everybody else on their actual actions (the same for
             every i), of [..., i, j, 0] the same with actor i on its MdR; zero on the diagonal;
             resp_full = clip((vm - va) / (vm + 1e-6), -1, 1) of their popcounts.  Needs fear=True
"""
from __future__ import annotations

import ctypes as C
import functools
import itertools
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .scenario import CompiledScenario, builtin


@dataclass
class StepResult:
    """What a step returned (views of the env's buffers, or of the ``into`` destinations).

    ``obs``: with the delta obs writer on (dense f32 obs; ``VecGridEnv.set_obs_delta``) the env
    patches a buffer it wrote last in place instead of rewriting it.  Writes to that buffer through
    torch ops are noticed (the tensor's version counter) and make the next step rewrite it in full;
    a write torch cannot see (a kernel or library given the raw pointer) must be followed by
    ``VecGridEnv.obs_dest_forget(buffer)`` before the env's next step into it."""
    obs: torch.Tensor
    reward: torch.Tensor
    fear: torch.Tensor
    shaped: torch.Tensor
    term: torch.Tensor
    trunc: torch.Tensor
    done: torch.Tensor
    mask: torch.Tensor
    crashes: torch.Tensor
    apples: torch.Tensor
    ep_return: torch.Tensor
    ep_fear: torch.Tensor
    ep_len: torch.Tensor
    final_obs: torch.Tensor | None = None
    actions: torch.Tensor | None = None
    mdr: torch.Tensor | None = None
    final_pos: torch.Tensor | None = None
    crash_bits: torch.Tensor | None = None
    restr_bits: torch.Tensor | None = None
    stats: torch.Tensor | None = None   # [rows, 8] per-block partial sums (_lib.STATS_NAMES)
    done_copy: torch.Tensor | None = None  # a second destination of done (step(into=...))
    stats_acc: torch.Tensor | None = None  # running per-block totals (step(into=...))
    tick: torch.Tensor | None = None       # += 1 per step (step(into=...))
    desc_copy: torch.Tensor | None = None  # [E, 12] int32 copy of the obs descriptors (step(into=...))
    fear_row: torch.Tensor | None = None   # [E, K, N] per-pair responsibility rows (fear_rows=True)
    fear_alt: torch.Tensor | None = None   # [E, K, 9] per-action counterfactual FeAR (fear_alt=True)
    feal: torch.Tensor | None = None       # [E, N] per-agent FeAL (feal=True)
    feal_valid: torch.Tensor | None = None  # [E, N, 2] int16 valid-action bit sets: others MdR / actual (feal=True)
    resp_full: torch.Tensor | None = None   # [E, N, N] responsibility matrix, every agent as actor (fear_full=True)
    resp_valid: torch.Tensor | None = None  # [E, N, N, 2] int16 valid-action bit sets: actor on MdR / actual


class StepGraph:
    """n captured VecGridEnv.step calls (VecGridEnv.capture_steps); replay() advances every env by
    n steps with one graph launch on the current stream."""

    def __init__(self, env, graph: torch.cuda.CUDAGraph):
        self.env, self.graph = env, graph

    def replay(self):
        self.graph.replay()
        self.env._replayed()


# obs destination pointer -> uid of the VecGridEnv that stepped into it last (VecGridEnv._guard_dest)
_DEST_WRITER: dict = {}
_UIDS = itertools.count(1)


def _ptr(t: torch.Tensor | None):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous()
    return t.data_ptr()


class VecGridEnv:
    def __init__(self, scenario: CompiledScenario | str = "level3", num_envs: int = 1, fear: bool = True,
                 fear_weight: float = -5.0, max_steps: int = 150, auto_reset: bool = True, seed: int = 42,
                 device: torch.device | int | None = None, env_offset: int = 0, final_obs: bool = False,
                 debug: bool = False, obs: bool = True, stats: bool = False, variant: int | str = 0,
                 obs_dtype: torch.dtype = torch.float32, fear_rows: bool = False,
                 fear_alt: bool = False, feal: bool = False, fear_full: bool = False):
        if not torch.cuda.is_available():
            raise _lib.GwError("VecGridEnv needs a HIP device (no CPU fallback by design)")
        sc = builtin(scenario) if isinstance(scenario, str) else scenario
        self.sc = sc
        self.E = int(num_envs)
        self.N, self.K, self.H, self.W = sc.N, sc.K, sc.H, sc.W
        self.fear_enabled = bool(fear)
        self.fear_weight = float(fear_weight)
        self.max_steps = int(max_steps)
        self.auto_reset = bool(auto_reset)
        self.seed = int(seed)
        # 0 / "multi": CustomMAEnv;  1 / "single": the single-agent CustomEnv (custom/customenv.py)
        self.variant = {"multi": 0, "single": 1}.get(variant, variant) if isinstance(variant, str) else int(variant)
        self.env_offset = int(env_offset)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else
                                   (device if isinstance(device, int) else device.index or 0))
        self.lib = _lib.load()

        keep = dict(region=np.ascontiguousarray(sc.region, np.uint8),
                    policy_id=np.ascontiguousarray(sc.policy_id, np.uint8),
                    cdf=np.ascontiguousarray(sc.policy_cdf, np.float64),
                    mdr=np.ascontiguousarray(sc.mdr, np.uint8),
                    apples=np.ascontiguousarray(sc.apples, np.int32))
        scn = _lib.GwScenario(sc.H, sc.W, keep["region"].ctypes.data, keep["policy_id"].ctypes.data,
                              int(sc.policy_cdf.shape[0]), keep["cdf"].ctypes.data, keep["mdr"].ctypes.data,
                              keep["apples"].ctypes.data)
        cfg = _lib.GwConfig(self.N, self.K, self.E, self.env_offset, int(self.fear_enabled), self.fear_weight,
                            self.max_steps, int(self.auto_reset), self.seed & 0xFFFFFFFFFFFFFFFF, self.variant)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gw_create(C.byref(scn), C.byref(cfg), self.device.index, C.byref(h)), "gw_create")
        self.handle = h
        if obs_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("obs_dtype: torch.float32 or torch.bfloat16")
        self.obs_dtype = obs_dtype
        if obs_dtype == torch.bfloat16:  # lossless: every obs value is exact in bf16
            _lib.check(self.lib.gw_set_obs_dtype(self.handle, 1), "gw_set_obs_dtype")
        if not obs and self.fear_enabled:
            # no full-obs writer to overlap: FeAR is on the step's critical path, where twice the
            # resident waves (32-env blocks) are faster (the local-window rollouts, profiles/r6_ab)
            _lib.check(self.lib.gw_set_fear_blocks(self.handle, 0), "gw_set_fear_blocks")

        dev, E, K, N = self.device, self.E, self.K, self.N
        f64 = dict(dtype=torch.float64, device=dev)
        self.out = dict(
            obs=torch.empty((K, E, sc.H, sc.W), dtype=obs_dtype, device=dev) if obs else None,
            final_obs=torch.full((K, E, sc.H, sc.W), float("nan"), dtype=obs_dtype, device=dev) if final_obs else None,
            reward=torch.zeros((E, K), **f64), fear=torch.zeros((E, K), **f64), shaped=torch.zeros((E, K), **f64),
            term=torch.zeros((E, K), dtype=torch.uint8, device=dev),
            trunc=torch.zeros((E, K), dtype=torch.uint8, device=dev),
            done=torch.zeros(E, dtype=torch.uint8, device=dev),
            mask=torch.zeros((E, K), dtype=torch.int16, device=dev),
            crashes=torch.zeros(E, dtype=torch.int32, device=dev),
            apples=torch.zeros(E, dtype=torch.int32, device=dev),
            ep_return=torch.zeros(E, **f64), ep_fear=torch.zeros(E, **f64),
            ep_len=torch.zeros(E, dtype=torch.int32, device=dev),
            actions=torch.zeros((E, N), dtype=torch.int32, device=dev) if debug else None,
            mdr=torch.zeros((E, N), dtype=torch.int32, device=dev) if debug else None,
            final_pos=torch.zeros((E, N), dtype=torch.int32, device=dev) if debug else None,
            crash_bits=torch.zeros(E, dtype=torch.uint8, device=dev) if debug else None,
            restr_bits=torch.zeros(E, dtype=torch.uint8, device=dev) if debug else None,
            stats=torch.zeros((int(self.lib.gw_stats_rows(self.handle)), _lib.GW_STATS), **f64) if stats else None,
            done_copy=None, stats_acc=None, tick=None, desc_copy=None,
            fear_row=torch.zeros((E, K, N), **f64) if fear_rows else None,
            # not a gw_step_out field: the env keeps the pointer (gw_set_fear_alt), so it has no step(into=...)
            fear_alt=torch.zeros((E, K, 9), **f64) if fear_alt else None,
            # the same (gw_set_feal)
            feal=torch.zeros((E, N), **f64) if feal else None,
            feal_valid=torch.zeros((E, N, 2), dtype=torch.int16, device=dev) if feal else None,
            # and (gw_set_fear_full)
            resp_full=torch.zeros((E, N, N), **f64) if fear_full else None,
            resp_valid=torch.zeros((E, N, N, 2), dtype=torch.int16, device=dev) if fear_full else None,
        )
        if fear_alt:
            _lib.check(self.lib.gw_set_fear_alt(self.handle, _ptr(self.out["fear_alt"])), "gw_set_fear_alt")
        self._step_out = _lib.GwStepOut(*[_ptr(self.out[n]) for n in _lib.STEP_OUT_FIELDS])
        self._into_cache = {}  # step(): (GwStepOut, fields, StepResult) per set of destination buffers
        self._into_sizes = None  # the destination sizes step(into=...) checks (built on first use)
        self._dev_index = self.device.index
        self._closed = False
        if feal or fear_full:
            try:
                if feal:
                    self.set_feal(self.out["feal"], self.out["feal_valid"])
                if fear_full:
                    self.set_fear_full(self.out["resp_full"], self.out["resp_valid"])
            except _lib.GwError:  # FeAR off: no record to compute them from
                self.close()
                raise
        self._obs_queued = False  # async obs: the last step's writer not yet launched / fenced
        # the delta obs writer (gw_set_obs_delta): on for dense f32 obs; GW_OBS_DELTA=0 keeps it off
        # (A/B; the results are the same).  _dest_guard: per obs destination the env wrote, what the
        # library's promise rests on (see _guard_dest)
        self._dest_guard = {}
        self._queued_dest = None  # lazy async obs: the obs destination of the writer still queued
        self._obs_lazy = False
        self._uid = next(_UIDS)
        self.obs_delta = False
        if obs and obs_dtype == torch.float32 and os.environ.get("GW_OBS_DELTA", "1") != "0":
            self.set_obs_delta(True)
        # GW_OBS_RIDE=0: the delta writer of an eager async step never runs inside the FeAR launch
        # (gw_set_obs_ride; A/B, the results are the same).  Only 0 or 1: the library refuses the rest
        ride = os.environ.get("GW_OBS_RIDE")
        if ride is not None:
            try:
                _lib.check(self.lib.gw_set_obs_ride(self.handle, int(ride) if ride in ("0", "1") else -1),
                           "gw_set_obs_ride (GW_OBS_RIDE)")
            except _lib.GwError:
                self.close()
                raise
        self.obs_async = False
        self.fear_async = False
        # the kernel path gw_create picked (GW_KERNEL, or by batch size: gw_kernel_path)
        self.kernel_path = ("v1", "split", "fused", "defer", "merged")[int(self.lib.gw_kernel_path(self.handle))]
        self.fused = self.kernel_path == "fused"

    # ------------------------------------------------------------------------------------
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def reset(self, spawn: torch.Tensor | None = None, env_mask: torch.Tensor | None = None):
        """CustomMAEnv.reset for all envs (or those with env_mask != 0).
        spawn: [E, N] int32 sorted road cells (replay) or None (device RNG)."""
        spawn = self._as_i32(spawn, (self.E, self.N))
        if env_mask is not None:
            env_mask = env_mask.to(device=self.device, dtype=torch.uint8).contiguous()
        self._guard_queued()  # the reset launches a queued (lazy) writer first
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gw_reset(self.handle, _ptr(env_mask), _ptr(spawn), _ptr(self.out["obs"]),
                                         _ptr(self.out["mask"]), self._stream()), "gw_reset")
        self._obs_queued = False
        self._queued_dest = None
        return self.out["obs"], self.out["mask"]

    _INTO_SPEC = {"obs": (torch.float32, "KEHW"), "final_obs": (torch.float32, "KEHW"),
                  "reward": (torch.float64, "EK"), "fear": (torch.float64, "EK"), "shaped": (torch.float64, "EK"),
                  "term": (torch.uint8, "EK"), "trunc": (torch.uint8, "EK"), "done": (torch.uint8, "E"),
                  "done_copy": (torch.uint8, "E"), "stats_acc": (torch.float64, "ROWS"),
                  "tick": (torch.int64, "ONE"), "desc_copy": (torch.int32, "DESC"),
                  "ep_return": (torch.float64, "E"), "fear_row": (torch.float64, "EKN")}

    def step(self, rl_actions: torch.Tensor | None = None, scripted: torch.Tensor | None = None,
             spawn: torch.Tensor | None = None, obs_out: torch.Tensor | None = None,
             final_obs_out: torch.Tensor | None = None, into: dict | None = None) -> StepResult:
        """rl_actions [E, K] int32 (None = uniform random RL policy on device);
        scripted [E, N-K] (replay) or None (scenario policy on device);
        spawn [E, N] spawns for auto-resetting envs (replay) or None;
        obs_out / final_obs_out: [K, E, H, W] float32 buffers to write this step's obs into
        instead of the env's own (e.g. a replay-ring slot: zero-copy replay storage);
        into: the same for any of obs, final_obs, reward, fear, shaped, term, trunc, done,
        done_copy (a second destination of done), ep_return, fear_row, stats_acc (per-block rows every
        step ADDS to: a running total), tick (int64 scalar, += 1 per step) (contiguous tensors of
        the output's dtype and size; e.g. the send buffer of parallel.ReturnGather)."""
        rl = self._as_i32(rl_actions, (self.E, self.K))
        sa = self._as_i32(scripted, (self.E, self.N - self.K))
        sp = self._as_i32(spawn, (self.E, self.N))
        over = dict(into or {})
        if obs_out is not None:
            over["obs"] = obs_out
        if final_obs_out is not None:
            over["final_obs"] = final_obs_out
        # the step's output struct and result per set of destination buffers, built once: a
        # pipelined step's host enqueue is on the critical path of short runs (the first step)
        key = tuple((n, t.data_ptr(), t.dtype, t.numel()) for n, t in over.items())
        cached = self._into_cache.get(key)
        if cached is None:
            cached = self._build_into(over)
            if len(self._into_cache) >= 4096:
                self._into_cache.clear()
            self._into_cache[key] = cached
        so, res, result = cached
        if self.obs_delta:
            self._guard_queued()  # lazy async obs: this gw_step launches the previous step's writer first
            if res["obs"] is not None:
                self._guard_dest(res["obs"])
        if torch.cuda.current_device() != self._dev_index:
            with torch.cuda.device(self.device):
                _lib.check(self.lib.gw_step(self.handle, _ptr(rl), _ptr(sa), _ptr(sp), C.byref(so),
                                            self._stream()), "gw_step")
        else:
            _lib.check(self.lib.gw_step(self.handle, _ptr(rl), _ptr(sa), _ptr(sp), C.byref(so),
                                        torch.cuda.current_stream().cuda_stream), "gw_step")
        self._obs_queued = self.obs_async and (res["obs"] is not None or res["final_obs"] is not None)
        self._queued_dest = res["obs"] if self._obs_queued and self._obs_lazy else None
        return result

    def _guard_queued(self):
        """Lazy async obs: the previous step's writer is still queued and is launched by the next
        gw_step, fence or reset, so its destination is vetted again right before that (a torch write
        since that step makes the queued writer a full one, as before the delta writer existed)."""
        if self._queued_dest is not None and self.obs_delta:
            self._guard_dest(self._queued_dest)

    def _guard_dest(self, t: torch.Tensor):
        """Keep the delta writer's promise (include/gridenv.h gw_set_obs_delta) for the obs
        destination ``t`` of the step about to run: the library may patch the buffer in place only
        if nothing but this env wrote it since the env's last step into it.  Per destination
        pointer the guard holds the tensor (so the allocator cannot hand its address to another
        tensor), its version counter (views share their base's: a ``copy_`` into any slot of a ring
        invalidates the whole ring, which is conservative), its storage and its size; if any of them
        differs now, the library forgets the destination first and this step rewrites it in full.
        A destination never seen is unknown to the library anyway.  At most GW_OBS_DESTS
        destinations are guarded; the least recently used is dropped (and forgotten by the library,
        whose table evicts by the same rule)."""
        ptr = t.data_ptr()
        g = self._dest_guard.get(ptr)
        if t.is_inference():  # no version counter to compare: never trusted
            self.obs_dest_forget(ptr)
            return
        # the last VecGridEnv of this process that stepped into ptr: another env's write is invisible
        # to torch's version counter too
        mine = _DEST_WRITER.get(ptr) == self._uid
        if not mine:
            if len(_DEST_WRITER) >= 4096:
                _DEST_WRITER.clear()  # every env then distrusts its destinations once
            _DEST_WRITER[ptr] = self._uid
        if g is not None:
            if mine and t._version == g[1] and (g[0] is t or (t.untyped_storage()._cdata == g[2] and
                                                              t.numel() == g[3])):
                g[0] = t  # (possibly another view of the same bytes)
                if len(self._dest_guard) >= _lib.GW_OBS_DESTS:  # full: keep the dict in order of use
                    self._dest_guard[ptr] = self._dest_guard.pop(ptr)
                return
            self.obs_dest_forget(ptr)
        elif len(self._dest_guard) >= _lib.GW_OBS_DESTS:
            self.obs_dest_forget(next(iter(self._dest_guard)))
        self._dest_guard[ptr] = [t, t._version, t.untyped_storage()._cdata, t.numel()]

    def set_obs_delta(self, enable: bool = True):
        """Turn the delta obs writer on / off (gw_set_obs_delta); either way every destination is
        forgotten, so the next step into any buffer writes it in full."""
        _lib.check(self.lib.gw_set_obs_delta(self.handle, int(bool(enable))), "gw_set_obs_delta")
        self._dest_guard.clear()
        self.obs_delta = bool(enable)

    def obs_dest_forget(self, dest: torch.Tensor | int | None = None):
        """Tell the env that something it cannot see wrote the obs buffer ``dest`` (a tensor or a
        device pointer; None: every buffer) since the env's last step into it: a kernel given the
        raw pointer, another library.  Writes through torch ops are seen by the env itself."""
        ptr = dest.data_ptr() if isinstance(dest, torch.Tensor) else dest
        _lib.check(self.lib.gw_obs_dest_forget(self.handle, ptr), "gw_obs_dest_forget")
        if ptr is None:
            self._dest_guard.clear()
        else:
            self._dest_guard.pop(ptr, None)

    def obs_delta_counts(self):
        """-> (full, delta): steps whose obs the full / the delta writer wrote (gw_obs_delta_counts)."""
        out = (C.c_int64 * 2)()
        _lib.check(self.lib.gw_obs_delta_counts(self.handle, out), "gw_obs_delta_counts")
        return int(out[0]), int(out[1])

    def obs_ride_count(self) -> int:
        """Steps whose delta obs writer ran inside the FeAR launch on the step's stream (gw_obs_ride_count)."""
        out = C.c_int64(0)
        _lib.check(self.lib.gw_obs_ride_count(self.handle, C.byref(out)), "gw_obs_ride_count")
        return int(out.value)

    def _build_into(self, over: dict):
        """(GwStepOut, result fields, StepResult) for the destination buffers ``over``."""
        so = self._step_out
        res = self.out
        if over:
            so = _lib.GwStepOut.from_buffer_copy(self._step_out)
            res = dict(self.out)
            sizes = self._into_sizes
            if sizes is None:
                sizes = self._into_sizes = {"KEHW": self.K * self.E * self.H * self.W, "EK": self.E * self.K,
                                            "E": self.E, "ONE": 1, "DESC": self.E * 12, "EKN": self.E * self.K * self.N,
                                            "ROWS": int(self.lib.gw_stats_rows(self.handle)) * _lib.GW_STATS}
            for name, t in over.items():
                dt, shp = self._INTO_SPEC[name]
                if shp == "KEHW":
                    dt = self.obs_dtype
                if t.dtype != dt or t.numel() != sizes[shp] or not t.is_contiguous() or t.device != self.device:
                    raise ValueError(f"step(into={name!r}): need a contiguous {dt} tensor of {sizes[shp]} elements "
                                     f"on {self.device}")
                setattr(so, name, _ptr(t))
                res[name] = t
        return so, res, StepResult(**res)

    def capture_steps(self, n: int, gather=None) -> "StepGraph":
        """Capture ``n`` consecutive ``step()`` calls (device RNG policies, no host inputs) into
        one HIP graph; each ``replay()`` then advances every env by n steps with a single launch
        from the host.  For the small-E regime, where a step is bound by its launch chain
        (C2: 4,096 envs), not by the GPU.  Nothing runs at capture time: the env's state is
        untouched until the first replay.

        gather: a parallel.ReturnGather with ``window == n`` and no steps pending (one rank):
        each captured step writes its returns into the gather's next slot and the window is
        compacted at the end of the graph, so every replay leaves the gather as it found it.
        HIP timing events cannot be recorded in a graph: profiling is switched off for the capture.

        Synchronous obs, or async obs on the merged kernel path: there every step is ONE
        step_obs launch (step t + the obs writer of step t-1, no events), so a capture of an EVEN
        number of steps that starts with the previous step's writer queued (at least one step
        since the last reset / fence, writing the same obs buffers as the captured steps) ends
        in the state it started from, and replays chain.  The defer path's async pipeline
        (cross-queue events between steps) cannot be captured."""
        if self.obs_async:
            if self.kernel_path != "merged":
                raise _lib.GwError("capture_steps: synchronous obs, or async obs on the merged path only")
            if n % 2 or not self._obs_queued:
                raise _lib.GwError("capture_steps (merged async obs): an even n, after a step (the previous "
                                   "step's obs writer queued)")
        if gather is not None and (gather.window != n or gather._fill != 0 or gather.distributed):
            raise _lib.GwError("capture_steps: the gather needs window == n, no pending steps and one rank")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            with _lib.graph_capture(g):
                self.profile(False)
                for i in range(n):
                    self.step(into=gather.into() if gather is not None else None)
                    if gather is not None:
                        gather.push()
        return StepGraph(self, g)

    def pipeline_save(self) -> bytes:
        """The host-side pipeline state (gw_pipeline_save): after capturing a graph of steps."""
        lib = self.lib
        buf = (C.c_char * int(lib.gw_pipeline_state_bytes()))()
        _lib.check(lib.gw_pipeline_save(self.handle, buf), "gw_pipeline_save")
        return bytes(buf)

    def pipeline_load(self, state: bytes, queued: bool | None = None):
        """Restore a pipeline_save state (after replaying the graph it was saved for; the next
        queued writer then runs on the current stream)."""
        buf = (C.c_char * len(state)).from_buffer_copy(state)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gw_pipeline_load(self.handle, buf, self._stream()), "gw_pipeline_load")
        self._obs_queued = self.obs_async if queued is None else bool(queued)

    def _replayed(self):
        """Host-side pipeline state after a StepGraph replay (gw_graph_replayed)."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gw_graph_replayed(self.handle, self._stream()), "gw_graph_replayed")
        self._obs_queued = self.obs_async

    def _as_i32(self, t, shape):
        if t is None:
            return None
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t))
        t = t.to(device=self.device, dtype=torch.int32).contiguous()
        if tuple(t.shape) != tuple(shape):
            t = t.reshape(shape)
        return t

    # ------------------------------------------------------------------------------------
    def state(self) -> dict:
        """Copy of the env state (device tensors): pos [N, E] cells, flags, t, episode,
        prev_dist [K, E], score, fear_score."""
        E, N, K, dev = self.E, self.N, self.K, self.device
        st = dict(pos=torch.empty((N, E), dtype=torch.int32, device=dev),
                  flags=torch.empty(E, dtype=torch.int32, device=dev),
                  t=torch.empty(E, dtype=torch.int32, device=dev),
                  episode=torch.empty(E, dtype=torch.int32, device=dev),
                  prev_dist=torch.empty((K, E), dtype=torch.int32, device=dev),
                  score=torch.empty(E, dtype=torch.float64, device=dev),
                  fear_score=torch.empty(E, dtype=torch.float64, device=dev))
        gs = _lib.GwState(*[_ptr(st[n]) for n in _lib.STATE_FIELDS])
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gw_copy_state(self.handle, C.byref(gs), 0, self._stream()), "gw_copy_state")
        return st

    def set_state(self, st: dict):
        gs = _lib.GwState(*[_ptr(st[n].contiguous()) if st.get(n) is not None else None
                            for n in _lib.STATE_FIELDS])
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gw_copy_state(self.handle, C.byref(gs), 1, self._stream()), "gw_copy_state")

    def fear_matrix(self, cells, actions, mdr=None, in_list=None) -> dict:
        """Responsibility.FeAR (full N x N matrix) and FeAL for n world snapshots of this env's map
        (gw_fear_matrix): cells / actions [n, N], mdr [n, N] or None (per-cell MdR), in_list [n]
        N-bit masks of the agents in ActionID4Agents or None (all).  -> device tensors resp
        [n, N, N] f64, vm, va [n, N, N] i32, feal [n, N] f64, feal_vm, feal_va [n, N] i32."""
        cells = torch.as_tensor(cells, device=self.device).to(torch.int32).contiguous()
        n, N = cells.shape[0], self.N
        assert cells.shape == (n, N)
        acts = self._as_i32(actions, (n, N))
        mdr = self._as_i32(mdr, (n, N))
        if in_list is not None:
            in_list = torch.as_tensor(in_list, device=self.device).to(torch.uint8).contiguous().reshape(n)
        dev = self.device
        out = dict(resp=torch.empty((n, N, N), dtype=torch.float64, device=dev),
                   vm=torch.empty((n, N, N), dtype=torch.int32, device=dev),
                   va=torch.empty((n, N, N), dtype=torch.int32, device=dev),
                   feal=torch.empty((n, N), dtype=torch.float64, device=dev),
                   feal_vm=torch.empty((n, N), dtype=torch.int32, device=dev),
                   feal_va=torch.empty((n, N), dtype=torch.int32, device=dev))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gw_fear_matrix(self.handle, n, _ptr(cells), _ptr(acts), _ptr(mdr), _ptr(in_list),
                                               *[_ptr(out[k]) for k in ("resp", "vm", "va", "feal", "feal_vm",
                                                                         "feal_va")], self._stream()),
                       "gw_fear_matrix")
        return out

    def set_feal(self, feal: torch.Tensor | None, feal_valid: torch.Tensor | None):
        """Arm (or, with both None, disarm) the per-agent FeAL outputs of the following steps
        (gw_set_feal): feal [E, N] float64, feal_valid [E, N, 2] int16; either may be None.  Raises
        on an env created with fear=False (no FeAR record to compute FeAL from)."""
        E, N = self.E, self.N
        for t, dt, n in ((feal, torch.float64, E * N), (feal_valid, torch.int16, 2 * E * N)):
            if t is not None and (t.dtype != dt or t.numel() != n or not t.is_contiguous() or t.device != self.device):
                raise ValueError(f"set_feal: need a contiguous {dt} tensor of {n} elements on {self.device}")
        _lib.check(self.lib.gw_set_feal(self.handle, _ptr(feal), _ptr(feal_valid)), "gw_set_feal")
        self.out["feal"], self.out["feal_valid"] = feal, feal_valid
        self._into_cache.clear()  # the cached StepResults carry the old views

    def set_fear_full(self, resp_full: torch.Tensor | None, resp_valid: torch.Tensor | None):
        """Arm (or, with both None, disarm) the N x N responsibility matrix of the following steps
        (gw_set_fear_full): resp_full [E, N, N] float64, resp_valid [E, N, N, 2] int16; either may be
        None.  Raises on an env created with fear=False (no FeAR record to compute it from)."""
        n = self.E * self.N * self.N
        for t, dt, m in ((resp_full, torch.float64, n), (resp_valid, torch.int16, 2 * n)):
            if t is not None and (t.dtype != dt or t.numel() != m or not t.is_contiguous() or t.device != self.device):
                raise ValueError(f"set_fear_full: need a contiguous {dt} tensor of {m} elements on {self.device}")
        _lib.check(self.lib.gw_set_fear_full(self.handle, _ptr(resp_full), _ptr(resp_valid)), "gw_set_fear_full")
        self.out["resp_full"], self.out["resp_valid"] = resp_full, resp_valid
        self._into_cache.clear()  # the cached StepResults carry the old views

    def copy_pos(self, out: torch.Tensor | None = None) -> torch.Tensor:
        """The agents' current cells into ``out`` ([N, E] int32, the env's pos layout; default: a new tensor):
        one device copy on the current stream (gw_copy_state with only pos set), capturable.  Called before
        ``step`` it holds that step's pre-move cells, what ``resp_map_accum`` bins by."""
        if out is None:
            out = torch.empty((self.N, self.E), dtype=torch.int32, device=self.device)
        if out.dtype != torch.int32 or out.numel() != self.N * self.E or not out.is_contiguous() or \
                out.device != self.device:
            raise ValueError(f"copy_pos: need a contiguous int32 tensor of {self.N * self.E} elements on {self.device}")
        gs = _lib.GwState(pos=_ptr(out))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gw_copy_state(self.handle, C.byref(gs), 0, self._stream()), "gw_copy_state")
        return out

    def resp_map_accum(self, resp_valid: torch.Tensor, cells: torch.Tensor, counts: torch.Tensor,
                       visits: torch.Tensor | None = None, active: torch.Tensor | None = None):
        """Bin one step's N x N valid-action sets by the agents' pre-move cells (gw_resp_map_accum,
        include/rollout_ops.h): for every env (``active[e] != 0`` if a mask is given) and ordered pair i != j,
        ``counts[0, cells[i, e], vm, va] += 1`` (caused at the actor's cell), ``counts[1, cells[j, e], vm, va] += 1``
        (received at the affected agent's cell) and ``visits[cells[i, e]] += 1`` once per (e, i).
        resp_valid: [E, N, N, 2] int16 (StepResult.resp_valid); cells: [N, E] int32 (``copy_pos`` before the
        step); counts: [2, H*W, 10, 10] int64 and visits: [H*W] int64 or None, both added to; active: [E] uint8
        or None.  ``marlnav.resp_map_from_counts`` turns the counts into the maps.  Raises on an env created
        without ``fear_full=True``."""
        if self.out.get("resp_valid") is None:
            raise ValueError("resp_map_accum needs VecGridEnv(fear_full=True) (the step's resp_valid sets)")
        E, N, HW = self.E, self.N, self.H * self.W
        for t, dt, n, name in ((resp_valid, torch.int16, 2 * E * N * N, "resp_valid"), (cells, torch.int32, N * E, "cells"),
                               (counts, torch.int64, 2 * HW * 100, "counts"), (visits, torch.int64, HW, "visits"),
                               (active, torch.uint8, E, "active")):
            if t is None and name in ("visits", "active"):
                continue
            if t is None or t.dtype != dt or t.numel() != n or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"resp_map_accum({name}=...): need a contiguous {dt} tensor of {n} elements on "
                                 f"{self.device}")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gw_resp_map_accum(_ptr(resp_valid), _ptr(cells), _ptr(active), _ptr(counts),
                                                  _ptr(visits), E, N, HW, self._stream()), "gw_resp_map_accum")

    def resp_footprint_accum(self, resp_valid: torch.Tensor, cells: torch.Tensor, actions: torch.Tensor,
                             counts: torch.Tensor, visits: torch.Tensor | None = None,
                             crash_bits: torch.Tensor | None = None, active: torch.Tensor | None = None,
                             radius: int = 5):
        """Bin one step's N x N valid-action sets by the actor's action and the affected agent's offset from the
        actor (gw_resp_footprint_accum, include/rollout_ops.h): for every env (``active[e] != 0`` if a mask is
        given) and ordered pair i != j, ``counts[0, actions[e, i], o, vm, va] += 1`` with o the bin of the offset
        (dr, dc) of ``cells[j, e]`` from ``cells[i, e]`` (the far bin beyond ``radius``), the same into
        ``counts[1]`` if bit j of ``crash_bits[e]`` is set, and ``visits[actions[e, i]] += 1`` once per (e, i).
        resp_valid: [E, N, N, 2] int16 (StepResult.resp_valid); cells: [N, E] int32 (``copy_pos`` before the
        step); actions: [E, N] int32 (StepResult.actions, an env created with ``debug=True``); counts:
        [2, 9, O, 10, 10] int64 with O = (2 radius + 1)^2 + 1 and visits: [9] int64 or None, both added to;
        crash_bits: [E] uint8 (StepResult.crash_bits) or None (plane 1 untouched); active: [E] uint8 or None;
        radius: 1..15.  ``marlnav.resp_footprint_from_counts`` turns the counts into the footprint.  Raises on
        an env created without ``fear_full=True``."""
        if self.out.get("resp_valid") is None:
            raise ValueError("resp_footprint_accum needs VecGridEnv(fear_full=True) (the step's resp_valid sets)")
        R = int(radius)
        if not 1 <= R <= 15:
            raise ValueError("resp_footprint_accum(radius=...): 1..15")
        E, N, O = self.E, self.N, (2 * R + 1) ** 2 + 1
        for t, dt, n, name in ((resp_valid, torch.int16, 2 * E * N * N, "resp_valid"), (cells, torch.int32, N * E, "cells"),
                               (actions, torch.int32, E * N, "actions"), (counts, torch.int64, 2 * 9 * O * 100, "counts"),
                               (visits, torch.int64, 9, "visits"), (crash_bits, torch.uint8, E, "crash_bits"),
                               (active, torch.uint8, E, "active")):
            if t is None and name in ("visits", "crash_bits", "active"):
                continue
            if t is None or t.dtype != dt or t.numel() != n or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"resp_footprint_accum({name}=...): need a contiguous {dt} tensor of {n} elements on "
                                 f"{self.device}")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gw_resp_footprint_accum(_ptr(resp_valid), _ptr(cells), _ptr(actions), _ptr(crash_bits),
                                                        _ptr(active), _ptr(counts), _ptr(visits), E, N, self.H, self.W,
                                                        R, self._stream()), "gw_resp_footprint_accum")

    def fear_preview(self, rl_actions: torch.Tensor | None = None, scripted: torch.Tensor | None = None,
                     out: torch.Tensor | None = None, actions: torch.Tensor | None = None,
                     mdr: torch.Tensor | None = None) -> torch.Tensor:
        """The per-action FeAR table of the step that ``step(rl_actions, scripted)`` would run next, without
        moving the world (gw_fear_preview): -> [E, K, 9] float64, what ``StepResult.fear_alt`` of that step
        would hold, bit for bit.  None arguments mean what they mean for ``step`` (the device-random RL policy /
        the scenario policy, with the step's own Philox counters).  Works with ``fear=False`` too.
        out: the [E, K, 9] float64 destination (default: a new tensor); actions / mdr: optional [E, N] int32
        outputs, the joint action that step will apply and the current cells' MdR.  Changes no env state."""
        E, K, N = self.E, self.K, self.N
        rl = self._as_i32(rl_actions, (E, K))
        sa = self._as_i32(scripted, (E, N - K))
        out = self._empty((E, K, 9), torch.float64) if out is None else out
        self._check_bufs("fear_preview", dict(out=out, actions=actions, mdr=mdr),
                         self._want_bufs("fear_preview", E, K, N), self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gw_fear_preview(self.handle, _ptr(rl), _ptr(sa), _ptr(out), _ptr(actions), _ptr(mdr),
                                                self._stream()), "gw_fear_preview")
        return out

    def fear_shield(self, table: torch.Tensor, actions: torch.Tensor, mask: torch.Tensor | None = None,
                    probs: torch.Tensor | None = None, tau: float = 0.0, agents: int | None = None,
                    out: torch.Tensor | None = None, flags: torch.Tensor | None = None):
        """The responsibility shield (gw_fear_shield): -> (actions [E, K] int32, flags [E, K] uint8).  An RL
        action whose previewed FeAR ``table[e, k, a]`` (``fear_preview`` of the proposed ``actions``) exceeds
        ``tau`` is replaced by an allowed one (mask bit set, FeAR <= tau): the most probable under ``probs``
        [K, E, 9] float32, or without probs the least FeAR; ties to the lowest action.  flags: 0 kept, 1
        replaced, 2 no allowed action and the least-FeAR masked one was the proposed one, 3 that one replaced
        it.  mask: [E, K] int16 9-bit action masks (None: all nine); agents: bitmask of the shielded RL agents
        (None: all K).  out may be ``actions`` itself.  The shield is unilateral: each row assumes the other
        agents keep their proposed actions (include/rollout_ops.h)."""
        E, K = self.E, self.K
        act = self._as_i32(actions, (E, K))
        out = self._empty((E, K), torch.int32) if out is None else out
        flags = self._empty((E, K), torch.uint8) if flags is None else flags
        self._check_bufs("fear_shield", dict(table=table, mask=mask, probs=probs, out=out, flags=flags),
                         self._want_bufs("fear_shield", E, K, self.N), self.device)
        bits = self._agent_bits(K, agents)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gw_fear_shield(_ptr(table), _ptr(act), _ptr(mask), _ptr(probs), E, K, float(tau), bits,
                                               _ptr(out), _ptr(flags), self._stream()), "gw_fear_shield")
        return out, flags

    def fear_shield_joint(self, rl_actions: torch.Tensor | None = None, scripted: torch.Tensor | None = None,
                          mask: torch.Tensor | None = None, probs: torch.Tensor | None = None, tau: float = 0.0,
                          agents: int | None = None, sweeps: int = 2, out: torch.Tensor | None = None,
                          flags: torch.Tensor | None = None, table: torch.Tensor | None = None,
                          joint: torch.Tensor | None = None):
        """The coordinated responsibility shield (gw_fear_shield_joint): -> (actions [E, K] int32, flags [E, K]
        uint8, table [E, K, 9] float64).  ``fear_preview`` + ``fear_shield`` composed over the shielded RL
        agents one after the other (ascending k, each visit on the table of the actions fixed so far), at most
        ``sweeps`` times round or until a sweep changes nothing, in one call; ``table`` is ``fear_preview`` of
        the joint action that ``step(actions, scripted)`` will apply, so ``table[e, k, actions[e, k]]`` is that
        step's ``fear[e, k]`` bit for bit.  flags: bit 0 replaced, bit 1 the last visit found no allowed action,
        bit 2 the agent is shielded and its entry exceeds tau, bit 3 the env's last sweep still changed
        something.  rl_actions / scripted as for ``fear_preview`` (None: the draws the step will make); mask,
        probs, tau, agents as for ``fear_shield``; out may be ``rl_actions`` itself; joint: optional [E, N]
        int32 output, the joint action of that step.  Changes no env state; works with ``fear=False``."""
        E, K, N = self.E, self.K, self.N
        rl = self._as_i32(rl_actions, (E, K))
        sa = self._as_i32(scripted, (E, N - K))
        self._check_sweeps("fear_shield_joint", sweeps)
        out = self._empty((E, K), torch.int32) if out is None else out
        flags = self._empty((E, K), torch.uint8) if flags is None else flags
        table = self._empty((E, K, 9), torch.float64) if table is None else table
        self._check_bufs("fear_shield_joint", dict(table=table, mask=mask, probs=probs, out=out, flags=flags, joint=joint),
                         self._want_bufs("fear_shield_joint", E, K, N), self.device)
        bits = self._agent_bits(K, agents)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gw_fear_shield_joint(self.handle, _ptr(rl), _ptr(sa), _ptr(mask), _ptr(probs),
                                                     float(tau), bits, int(sweeps), _ptr(out), _ptr(flags),
                                                     _ptr(table), _ptr(joint), self._stream()),
                       "gw_fear_shield_joint")
        return out, flags, table

    def crash_shield_joint(self, actions: torch.Tensor | None = None, scripted: torch.Tensor | None = None, *,
                           mask: torch.Tensor | None = None, probs: torch.Tensor | None = None,
                           tau: float | None = None, agents: int | None = None, sweeps: int = 2,
                           out: torch.Tensor | None = None, flags: torch.Tensor | None = None,
                           table: torch.Tensor | None = None, joint: torch.Tensor | None = None,
                           outcome: torch.Tensor | None = None, outcome_prop: torch.Tensor | None = None,
                           crash9: torch.Tensor | None = None) -> dict:
        """The coordinated crash-aware shield (gw_crash_shield_joint): ``step_preview``'s safe masks inside
        ``fear_shield_joint``'s sweeps, in one call.  The shielded RL agents are visited one after the other
        (ascending k, at most ``sweeps`` times round or until a sweep changes nothing); a visit previews the agent's
        nine actions with the real world update against the actions fixed so far, takes the crashing ones out of
        its mask (unless all crash) and picks as ``fear_shield`` does.  ``tau=None`` is the crash shield alone (a
        zero table under tau = 0: only an agent that would crash is moved, to its most probable safe action);
        a float adds FeAR.  -> a dict of tensors (given, or new ones):
          "actions" [E, K] int32 (``out``; may be ``actions`` itself), "flags" [E, K] uint8: bits 0-3 as
            ``fear_shield_joint`` (bit 2 only with a tau), bit 4 the agent crashes in the step that applies
            "actions", bit 5 every masked action of the agent's last visit crashed it (unavoidable);
          "table" [E, K, 9] float64: ``fear_preview`` of the applied joint action (with a tau, or when ``table``
            is given; else absent and no FeAR world update runs);
          "joint" [E, N] int32 (only when given), "outcome" / "outcome_prop" [E] int16: crash bits | restricted
            bits << 8 of the step that applies "actions" / of the proposal, "crash9" [E, K] int16: the own-crash
            sets under the applied joint action (``step_preview``'s).
        actions / scripted as for ``fear_preview`` (None: the draws the step will make); mask, probs, agents as for
        ``fear_shield``.  Changes no env state; works with ``fear=False``."""
        E, K, N = self.E, self.K, self.N
        self._check_crash_shield_args(E, K, N, actions, scripted, sweeps,
                                      dict(mask=mask, probs=probs, out=out, flags=flags, table=table, joint=joint,
                                           outcome=outcome, outcome_prop=outcome_prop, crash9=crash9), self.device)
        rl = self._as_i32(actions, (E, K))
        sa = self._as_i32(scripted, (E, N - K))
        use_fear = tau is not None
        out = self._empty((E, K), torch.int32) if out is None else out
        flags = self._empty((E, K), torch.uint8) if flags is None else flags
        table = self._empty((E, K, 9), torch.float64) if table is None and use_fear else table
        outcome = self._empty((E,), torch.int16) if outcome is None else outcome
        outcome_prop = self._empty((E,), torch.int16) if outcome_prop is None else outcome_prop
        crash9 = self._empty((E, K), torch.int16) if crash9 is None else crash9
        bits = self._agent_bits(K, agents)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gw_crash_shield_joint(self.handle, _ptr(rl), _ptr(sa), _ptr(mask), _ptr(probs),
                                                      int(use_fear), float(tau) if use_fear else 0.0, bits,
                                                      int(sweeps), _ptr(out), _ptr(flags), _ptr(table), _ptr(joint),
                                                      _ptr(outcome), _ptr(outcome_prop), _ptr(crash9), self._stream()),
                       "gw_crash_shield_joint")
        res = dict(actions=out, flags=flags, outcome=outcome, outcome_prop=outcome_prop, crash9=crash9)
        return {**res, **{n: t for n, t in (("table", table), ("joint", joint)) if t is not None}}

    def _empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    @staticmethod
    def _agent_bits(K: int, agents):  # the shields' ``agents`` as the library's bitmask (None: all K RL agents)
        return (1 << K) - 1 if agents is None else int(agents) & 0xFFFFFFFF

    @staticmethod
    def _check_sweeps(who: str, sweeps):
        if not 1 <= int(sweeps) <= 8:
            raise ValueError(f"{who}(sweeps=...): 1..8 (GW_SHIELD_MAX_SWEEPS)")

    @staticmethod
    def _check_counts(who: str, **given):  # argument name = (array-like or None, the elements it must hold)
        for name, (t, n) in given.items():
            if t is not None and int(np.prod(np.shape(t))) != n:
                raise ValueError(f"{who}({name}=...): need {n} elements, got shape {tuple(np.shape(t))}")

    @staticmethod
    @functools.lru_cache(maxsize=None)  # a per-step call path: the table is built once per method and shape
    def _want_bufs(who: str, E: int, K: int, N: int) -> dict:
        """(dtype, elements) of the buffers that method ``who`` takes, by argument name (_check_bufs' ``want``)."""
        if who == "fear_preview":
            return dict(out=(torch.float64, E * K * 9), actions=(torch.int32, E * N), mdr=(torch.int32, E * N))
        return dict(mask=(torch.int16, E * K), probs=(torch.float32, K * E * 9), out=(torch.int32, E * K),
                    flags=(torch.uint8, E * K), table=(torch.float64, E * K * 9), joint=(torch.int32, E * N),
                    outcome=(torch.int16, E), outcome_prop=(torch.int16, E), crash9=(torch.int16, E * K))

    @staticmethod
    def _check_bufs(who: str, bufs: dict, want: dict, device=None, note: str = ""):
        """The buffer check of the preview and shield methods (``who``: the method's name): every tensor of ``bufs``
        (argument name -> tensor; None: not given) has the dtype and the element count of ``want[name]``, is
        contiguous and, if a ``device`` is given, lies on it; else ValueError naming the method and the argument."""
        for name, t in bufs.items():
            dt, n = want[name]
            if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == dt and t.numel() == n
                                      and t.is_contiguous() and (device is None or t.device == device)):
                raise ValueError(f"{who}({name}=...): need a contiguous {dt} tensor of {n} elements"
                                 + (f" on {device}" if device is not None else "") + note)

    @staticmethod
    def _check_crash_shield_args(E: int, K: int, N: int, actions, scripted, sweeps, bufs: dict, device=None):
        """The argument checks of ``crash_shield_joint`` (ValueError before the call; no device needed when
        ``device`` is None): shapes, dtypes, contiguity and the sweep count."""
        VecGridEnv._check_counts("crash_shield_joint", actions=(actions, E * K), scripted=(scripted, E * (N - K)))
        VecGridEnv._check_sweeps("crash_shield_joint", sweeps)
        VecGridEnv._check_bufs("crash_shield_joint", bufs, VecGridEnv._want_bufs("crash_shield_joint", E, K, N), device)

    @staticmethod
    def _check_step_preview_args(E: int, K: int, N: int, rl_actions, scripted, mask):
        """The argument checks of ``step_preview`` that need no device: shapes and the mask's dtype."""
        VecGridEnv._check_counts("step_preview", rl_actions=(rl_actions, E * K), scripted=(scripted, E * (N - K)))
        VecGridEnv._check_bufs("step_preview", dict(mask=mask), dict(mask=(torch.int16, E * K)),
                               note=" (the 9-bit action masks, as StepResult.mask)")

    def step_preview(self, rl_actions: torch.Tensor | None = None, scripted: torch.Tensor | None = None,
                     mask: torch.Tensor | None = None, reward: bool = True) -> dict:
        """The step outcome preview (gw_step_preview): what ``step(rl_actions, scripted)`` would do under each of
        the nine actions of each RL agent, without moving the world.  -> a dict of tensors, allocated once and
        reused by every call:
          "outcome" [E, K, 9] int16: bits 0-7 the crash bits of all N agents, bits 8-15 the restricted bits of the
            real world update with agent k playing a and everybody else the action the step will apply;
          "reward_alt" [E, K, 9] float64 (``reward=True``): the env reward that step would pay agent k, bit for bit;
          "crash9" [E, K] int16: bit a = agent k itself crashes under a;
          "safe_mask" [E, K] int16: ``mask & ~crash9`` (mask None: all nine), or ``mask`` where that is empty;
          "actions" [E, N] int32: the joint action that step will apply.
        None arguments mean what they mean for ``step``.  Works with ``fear=False``.  Changes no env state.  The
        preview is unilateral: every entry assumes that the other agents play their proposed actions."""
        E, K, N = self.E, self.K, self.N
        self._check_step_preview_args(E, K, N, rl_actions, scripted, mask)
        rl = self._as_i32(rl_actions, (E, K))
        sa = self._as_i32(scripted, (E, N - K))
        if mask is not None and mask.device != self.device:
            raise ValueError(f"step_preview(mask=...): need a tensor on {self.device}")
        buf = getattr(self, "_step_preview_out", None)
        if buf is None:
            i16 = dict(dtype=torch.int16, device=self.device)
            buf = dict(outcome=torch.zeros((E, K, 9), **i16), reward_alt=None,
                       crash9=torch.zeros((E, K), **i16), safe_mask=torch.zeros((E, K), **i16),
                       actions=torch.zeros((E, N), dtype=torch.int32, device=self.device))
            self._step_preview_out = buf
        if reward and buf["reward_alt"] is None:
            buf["reward_alt"] = torch.zeros((E, K, 9), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gw_step_preview(self.handle, _ptr(rl), _ptr(sa), _ptr(mask), _ptr(buf["outcome"]),
                                                _ptr(buf["reward_alt"]) if reward else None, _ptr(buf["crash9"]),
                                                _ptr(buf["safe_mask"]), _ptr(buf["actions"]), self._stream()),
                       "gw_step_preview")
        return {n: t for n, t in buf.items() if t is not None and (reward or n != "reward_alt")}

    def step_lookahead(self, rl_actions: torch.Tensor | None = None, scripted: torch.Tensor | None = None,
                       mask: torch.Tensor | None = None) -> dict:
        """The two-step crash lookahead (gw_step_lookahead): ``step_preview``'s own-crash sets for the step that
        ``step(rl_actions, scripted)`` would run and for the step after it, without moving the world.  -> a dict of
        tensors, allocated once and reused by every call:
          "crash2" [E, K, 9] int16: bit b of entry (k, a) = agent k itself crashes in the step after, playing b
            from the cell that first action a leaves it in, while the other RL agents stay (action 0) and the
            scripted agents play their draws of that step; 0 where the step ends the episode under a;
          "ends" [E, K] int16: bit a = the step ends the episode with agent k playing a (another RL agent's crash
            and the step cap included);
          "crash9" [E, K] int16: ``step_preview``'s, bit a = agent k itself crashes in the step under a;
          "trap9" [E, K] int16: bit a = the step goes on under a and every action the cell after it allows
            crashes k;
          "ahead_mask" [E, K] int16: ``mask & ~crash9 & ~trap9`` (mask None: all nine); where that is empty,
            ``step_preview``'s safe mask;
          "actions" [E, N] int32: the joint action that step will apply.
        None arguments mean what they mean for ``step``; a ``scripted`` override holds for the first step only.
        Works with ``fear=False``.  Changes no env state."""
        E, K, N = self.E, self.K, self.N
        self._check_counts("step_lookahead", rl_actions=(rl_actions, E * K), scripted=(scripted, E * (N - K)))
        self._check_bufs("step_lookahead", dict(mask=mask), dict(mask=(torch.int16, E * K)), self.device,
                         note=" (the 9-bit action masks, as StepResult.mask)")
        rl = self._as_i32(rl_actions, (E, K))
        sa = self._as_i32(scripted, (E, N - K))
        buf = getattr(self, "_step_lookahead_out", None)
        if buf is None:
            i16 = dict(dtype=torch.int16, device=self.device)
            buf = dict(crash2=torch.zeros((E, K, 9), **i16), ends=torch.zeros((E, K), **i16),
                       crash9=torch.zeros((E, K), **i16), trap9=torch.zeros((E, K), **i16),
                       ahead_mask=torch.zeros((E, K), **i16),
                       actions=torch.zeros((E, N), dtype=torch.int32, device=self.device))
            self._step_lookahead_out = buf
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gw_step_lookahead(self.handle, _ptr(rl), _ptr(sa), _ptr(mask), _ptr(buf["crash2"]),
                                                  _ptr(buf["ends"]), _ptr(buf["crash9"]), _ptr(buf["trap9"]),
                                                  _ptr(buf["ahead_mask"]), _ptr(buf["actions"]), None,
                                                  self._stream()), "gw_step_lookahead")
        return dict(buf)

    def step_horizon(self, rl_actions: torch.Tensor | None = None, scripted: torch.Tensor | None = None,
                     mask: torch.Tensor | None = None, horizon: int = 3) -> dict:
        """The crash horizon (gw_step_horizon): for each RL agent and first action, how many of the next ``horizon``
        steps (2..4) the agent can survive, without moving the world.  -> a dict of tensors, allocated once and
        reused by every call:
          "depth" [E, K, 9] uint8 in 0..horizon: the largest d such that some continuation keeps agent k from
            crashing in the steps 1..d after first action a; after the first step the other RL agents stay
            (action 0), the scripted agents play their draws, and k plays what its cell's action mask allows.  An
            episode end without k's own crash counts as ``horizon``;
          "ends" / "crash9" [E, K] int16: ``step_lookahead``'s, bit for bit;
          "viable9" [E, K] int16: bit a = depth == horizon;
          "horizon_mask" [E, K] int16: the actions of ``mask`` (None: all nine) whose depth is the largest over
            the mask; at horizon 2 it is ``step_lookahead``'s "ahead_mask";
          "actions" [E, N] / "mdr" [E, N] int32: the joint action that step will apply and the cells' MdR.
        None arguments mean what they mean for ``step``; a ``scripted`` override holds for the first step only.
        Works with ``fear=False``.  Changes no env state."""
        E, K, N = self.E, self.K, self.N
        if isinstance(horizon, bool) or not 2 <= int(horizon) <= 4:
            raise ValueError("step_horizon(horizon=...): an int in 2..4 (GW_HORIZON_MAX)")
        self._check_counts("step_horizon", rl_actions=(rl_actions, E * K), scripted=(scripted, E * (N - K)))
        self._check_bufs("step_horizon", dict(mask=mask), dict(mask=(torch.int16, E * K)), self.device,
                         note=" (the 9-bit action masks, as StepResult.mask)")
        rl = self._as_i32(rl_actions, (E, K))
        sa = self._as_i32(scripted, (E, N - K))
        buf = getattr(self, "_step_horizon_out", None)
        if buf is None:
            i16 = dict(dtype=torch.int16, device=self.device)
            i32 = dict(dtype=torch.int32, device=self.device)
            buf = dict(depth=torch.zeros((E, K, 9), dtype=torch.uint8, device=self.device),
                       ends=torch.zeros((E, K), **i16), crash9=torch.zeros((E, K), **i16),
                       viable9=torch.zeros((E, K), **i16), horizon_mask=torch.zeros((E, K), **i16),
                       actions=torch.zeros((E, N), **i32), mdr=torch.zeros((E, N), **i32))
            self._step_horizon_out = buf
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gw_step_horizon(self.handle, _ptr(rl), _ptr(sa), _ptr(mask), int(horizon),
                                                _ptr(buf["depth"]), _ptr(buf["ends"]), _ptr(buf["crash9"]),
                                                _ptr(buf["viable9"]), _ptr(buf["horizon_mask"]), _ptr(buf["actions"]),
                                                _ptr(buf["mdr"]), self._stream()), "gw_step_horizon")
        return dict(buf)

    def step_plan(self, rl_actions: torch.Tensor | None = None, scripted: torch.Tensor | None = None,
                  mask: torch.Tensor | None = None, horizon: int = 3) -> dict:
        """The reward horizon (gw_step_plan): for each RL agent and first action, how many of the next ``horizon``
        steps (2..4) the agent can survive and the most env reward those steps can pay it, without moving the
        world.  ``step_horizon`` on the world with its real apples: after the first step the other RL agents stay
        (action 0), the scripted agents play their draws, k plays what its cell's action mask allows, and every step
        is the real world update with the step's own reward and ``done`` rules (eating the last apple ends the
        episode).  -> a dict of tensors, allocated once and reused by every call:
          "depth" [E, K, 9] uint8 in 0..horizon: ``step_horizon``'s definition on that world;
          "ret" [E, K, 9] int16, in tenths of a reward unit: the largest sum of env rewards over the continuations
            that reach "depth" (survival first, return second); a continuation below ``horizon`` includes its one
            crash (-100);
          "path" [E, K, 9, 3] uint8: the actions after a of the continuation that attains ("depth", "ret"), ties to
            the lowest action; the crash step or the step that ends the episode is its last entry, 0xFF after it;
          "ends" / "crash9" [E, K] int16: ``step_horizon``'s, bit for bit;
          "plan_mask" [E, K] int16: the actions of ``mask`` (None: all nine) whose ("depth", "ret") is the
            lexicographic maximum over the mask;
          "actions" [E, N] / "mdr" [E, N] int32: the joint action that step will apply and the cells' MdR.
        None arguments mean what they mean for ``step``; a ``scripted`` override holds for the first step only.
        Works with ``fear=False``.  Changes no env state."""
        E, K, N = self.E, self.K, self.N
        if isinstance(horizon, bool) or not 2 <= int(horizon) <= 4:
            raise ValueError("step_plan(horizon=...): an int in 2..4 (GW_HORIZON_MAX)")
        self._check_counts("step_plan", rl_actions=(rl_actions, E * K), scripted=(scripted, E * (N - K)))
        self._check_bufs("step_plan", dict(mask=mask), dict(mask=(torch.int16, E * K)), self.device,
                         note=" (the 9-bit action masks, as StepResult.mask)")
        rl = self._as_i32(rl_actions, (E, K))
        sa = self._as_i32(scripted, (E, N - K))
        buf = getattr(self, "_step_plan_out", None)
        if buf is None:
            i16 = dict(dtype=torch.int16, device=self.device)
            i32 = dict(dtype=torch.int32, device=self.device)
            u8 = dict(dtype=torch.uint8, device=self.device)
            buf = dict(depth=torch.zeros((E, K, 9), **u8), ret=torch.zeros((E, K, 9), **i16),
                       path=torch.zeros((E, K, 9, 3), **u8), ends=torch.zeros((E, K), **i16),
                       crash9=torch.zeros((E, K), **i16), plan_mask=torch.zeros((E, K), **i16),
                       actions=torch.zeros((E, N), **i32), mdr=torch.zeros((E, N), **i32))
            self._step_plan_out = buf
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gw_step_plan(self.handle, _ptr(rl), _ptr(sa), _ptr(mask), int(horizon),
                                             _ptr(buf["depth"]), _ptr(buf["ret"]), _ptr(buf["path"]), _ptr(buf["ends"]),
                                             _ptr(buf["crash9"]), _ptr(buf["plan_mask"]), _ptr(buf["actions"]),
                                             _ptr(buf["mdr"]), self._stream()), "gw_step_plan")
        return dict(buf)

    def obs_patch(self, size: int, final: bool = False, out: torch.Tensor | None = None,
                  final_out: torch.Tensor | None = None):
        """Egocentric local observations (gw_obs_patch): [K, E, size, size] float32, agent k's obs
        cropped to the size x size window centred on its own cell, cells outside the grid -1.
        An opt-in input format (the reference observes the whole grid); derived from the obs
        descriptors, so the env may run without dense obs (``obs=False``).  final=True also
        returns the terminal-obs patches of the envs done at the last step: (patch, final)."""
        K, E, P = self.K, self.E, int(size)
        if out is None:
            out = torch.empty((K, E, P, P), dtype=torch.float32, device=self.device)
        if final and final_out is None:
            final_out = torch.full((K, E, P, P), float("nan"), dtype=torch.float32, device=self.device)
        for t in (out, final_out):
            if t is not None and (t.dtype != torch.float32 or t.numel() != K * E * P * P or not t.is_contiguous()):
                raise ValueError(f"obs_patch: need contiguous float32 [K, E, {P}, {P}] buffers")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gw_obs_patch(self.handle, P, _ptr(out), _ptr(final_out) if final else None,
                                             self._stream()), "gw_obs_patch")
        return (out, final_out) if final else out

    def patch_next(self, size: int, out: torch.Tensor, final_out: torch.Tensor | None = None):
        """Have the next ``step`` write its P x P windows into ``out`` / ``final_out`` exactly as
        ``obs_patch(size, final=True, out=out, final_out=final_out)`` right after it would
        (gw_step_patch_next): with FeAR on, inside the FeAR launch where the row writer applies."""
        K, E, P = self.K, self.E, int(size)
        for t in (out, final_out):
            if t is not None and (t.dtype != torch.float32 or t.numel() != K * E * P * P or not t.is_contiguous()):
                raise ValueError(f"patch_next: need contiguous float32 [K, E, {P}, {P}] buffers")
        _lib.check(self.lib.gw_step_patch_next(self.handle, P, _ptr(out), _ptr(final_out)), "gw_step_patch_next")

    def set_obs_async(self, enable: bool | str = True, fear_async: bool = False):
        """Pipeline the obs writer of step t with the world update of step t+1 (gw_set_obs_async).
        While on, ``step``'s obs / final_obs are ready on the current stream only after
        ``obs_fence()`` (rewards, dones, masks and state are ordered as usual).
        enable="lazy": the writer is launched at the next step, behind the caller's work between
        the steps (an actor kernel), instead of right after the world update.
        fear_async (defer path, FeAR on): the FeAR-owned outputs (fear, shaped, ep_return,
        ep_fear, fear_row, fear_alt, feal, feal_valid, resp_full, resp_valid, the FeAR stats rows) are ready only after ``fear_fence()``, so the caller's next
        work (the fused actor) overlaps the FeAR kernel."""
        mode = 2 if enable == "lazy" else int(bool(enable))
        if mode and fear_async:
            mode |= 4
        self._guard_queued()  # switching the pipeline off launches a queued (lazy) writer
        _lib.check(self.lib.gw_set_obs_async(self.handle, mode), "gw_set_obs_async")
        if not mode:
            self._obs_queued = False
            self._queued_dest = None
        self._obs_lazy = bool(mode & 2)
        self.obs_async = bool(mode)
        self.fear_async = bool(mode & 4)

    def obs_fence(self):
        """Order the last step's outputs (obs, and FeAR-owned ones) before later work on the
        current stream (async mode)."""
        if self.obs_async:
            self._guard_queued()  # the fence launches a queued (lazy) writer
            with torch.cuda.device(self.device):
                _lib.check(self.lib.gw_obs_fence(self.handle, self._stream()), "gw_obs_fence")
            self._obs_queued = False
            self._queued_dest = None

    def fear_fence(self):
        """Order the last step's FeAR-owned outputs before later work on the current stream."""
        if self.fear_async:
            with torch.cuda.device(self.device):
                _lib.check(self.lib.gw_fear_fence(self.handle, self._stream()), "gw_fear_fence")

    def profile(self, enable: bool = True, reserve: int = 0):
        """Time each gw_step kernel with HIP events (see gw_profile); reserve: create that many
        timing events now, outside any timed region."""
        _lib.check(self.lib.gw_profile(self.handle, max(int(enable), int(reserve)) if enable else 0), "gw_profile")

    def count_sims(self, counter: torch.Tensor | None):
        """Count the FeAR counterfactual world updates (de-duplicated sims, gw_count_sims) of the
        following steps into ``counter`` (int64 [1] on the env's device; None stops counting)."""
        if counter is not None:
            assert counter.dtype == torch.int64 and counter.device == self.device and counter.numel() >= 1
        _lib.check(self.lib.gw_count_sims(self.handle, counter.data_ptr() if counter is not None else None),
                   "gw_count_sims")

    def profile_spans(self):
        """-> float64 [n, 3] (kind, start ms, end ms) of every timed launch since the last
        profile_read (gw_profile_spans; call before profile_read, which clears them)."""
        import numpy as np
        n = C.c_int64()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gw_profile_spans(self.handle, None, 0, C.byref(n)), "gw_profile_spans")
            buf = (C.c_double * (3 * max(n.value, 1)))()
            _lib.check(self.lib.gw_profile_spans(self.handle, buf, n.value, C.byref(n)), "gw_profile_spans")
        return np.frombuffer(buf, dtype=np.float64)[: 3 * n.value].reshape(-1, 3).copy()

    def profile_read(self):
        """-> (ms summed over timed steps [step_kernel, obs_kernel, fear_kernel], timed steps).
        fear_kernel is nonzero only with GW_KERNEL=defer (it overlaps obs_kernel there)."""
        ms = (C.c_double * 3)()
        n = C.c_int64()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gw_profile_read(self.handle, ms, C.byref(n)), "gw_profile_read")
        return (ms[0], ms[1], ms[2]), n.value

    def positions(self) -> torch.Tensor:
        return self.state()["pos"].t().contiguous()

    def close(self):
        if not self._closed and getattr(self, "handle", None):
            self.lib.gw_destroy(self.handle)
            self._closed = True

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
