"""Checkpoints of chains that run in segments (include/mcq.h: mcq_resume, mcq_checkpoint_device).

A Checkpoint holds what defines a run (N, chain type, Q, the schedule(s) and the length of the WHOLE schedule, the seeds, the trace
mode), how many steps are done, and per chain the placement, the MT19937 state as np.random.get_state() holds it, the energy, and the
running summary of the whole run so far (best energy / state / step, accepted steps, near ties, words taken from the stream).  The segments come
from the GPU (experiments.start_chains / continue_chains / warm_start_chains); merging them is plain NumPy and lives here.

The merge rules follow from what the reference reports for one unbroken chain (experiments.py:329-365): best_energy is
min(energy_history), steps_to_best the FIRST index of that minimum, so a later segment moves them only by a strictly lower energy.
"""
import json

import numpy as np

from . import abi

FORMAT = 1
_PER_CHAIN = ("state", "stream_state", "energy", "best_energy", "best_state", "steps_to_best", "n_accepted", "stream_words", "near_ties")


class Checkpoint:
    def __init__(self, N, mcmc_type, schedule_steps, seeds, schedule_params=None, schedule_sets=None, chains_per_set=None, Q=None,
                 trace=True):
        if (schedule_params is None) == (schedule_sets is None):
            raise ValueError("a checkpoint names one schedule (schedule_params) or several (schedule_sets)")
        self.N = int(N)
        self.mode = "board" if abi.mode_of(mcmc_type) == abi.MODE_BOARD else "full_3d"
        self.Q = self.N * self.N if Q is None else int(Q)
        self.schedule_params = None if schedule_params is None else dict(schedule_params)
        self.schedule_sets = None if schedule_sets is None else [dict(sp) for sp in schedule_sets]
        self.chains_per_set = None if chains_per_set is None else int(chains_per_set)
        self.schedule_steps = int(schedule_steps)
        self.seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
        self.trace = trace
        self.step = 0
        for k in _PER_CHAIN:
            setattr(self, k, None)

    @property
    def n_chains(self):
        return len(self.seeds)

    def require(self, N=None, mcmc_type=None, Q=None):
        """Raises ValueError unless the checkpoint is one of chains of this size, type and queen count."""
        if N is not None and int(N) != self.N:
            raise ValueError(f"the checkpoint holds chains of N = {self.N}, not N = {N}")
        if mcmc_type is not None and ("board" if abi.mode_of(mcmc_type) == abi.MODE_BOARD else "full_3d") != self.mode:
            raise ValueError(f"the checkpoint holds {self.mode} chains, not {mcmc_type}")
        if Q is not None and int(Q) != self.Q:
            raise ValueError(f"the checkpoint holds chains of Q = {self.Q} queens, not Q = {Q}")

    def params(self, n_steps, trace=True, lanes_per_chain=0, flags=0, init_mode="random", init_modes=None):
        """The Params block of a segment of `n_steps` steps of these chains (early stopping off: it cannot be continued)."""
        kw = dict(mcmc_type=self.mode, early_stop_patience=None, trace=trace, flags=flags, lanes_per_chain=lanes_per_chain)
        if self.schedule_sets is not None:
            if self.Q != self.N * self.N:
                raise ValueError("schedule sets run Q = N^2 queens")
            return abi.make_params_sets(self.N, n_steps, init_mode, self.schedule_sets, self.chains_per_set, init_modes=init_modes, **kw)
        return abi.make_params(self.N, n_steps, init_mode, self.schedule_params, self.n_chains, Q=self.Q, **kw)

    def merge(self, seg, seg_steps):
        """Take in the result of the segment that ran steps [self.step, self.step + seg_steps): a dict with initial_energy, final_energy,
        best_energy, steps_to_best and n_accepted per chain and, where the segment has them, best_state, final_state, stream_state,
        stream_words and near_ties (which add up, like n_accepted).  Raises ValueError when the segment did not start where the checkpoint stands."""
        seg_steps = int(seg_steps)
        if seg_steps < 0 or self.step + seg_steps > self.schedule_steps:
            raise ValueError(f"a segment of {seg_steps} steps from step {self.step} leaves the schedule of {self.schedule_steps} steps")
        e0 = np.asarray(seg["initial_energy"]).astype(np.int64)
        if e0.shape != (self.n_chains,):
            raise ValueError("the segment holds another number of chains")
        sbest, sstb = np.asarray(seg["best_energy"]).astype(np.int64), np.asarray(seg["steps_to_best"]).astype(np.int64)
        if self.energy is None:  # the first segment: its summary is the run's
            self.best_energy, self.steps_to_best = sbest.copy(), sstb + self.step
            self.n_accepted = np.asarray(seg["n_accepted"]).astype(np.int64).copy()
            self.stream_words = np.zeros(self.n_chains, dtype=np.uint64)
            if seg.get("near_ties") is not None:  # counted from the first segment on, or not at all
                self.near_ties = np.asarray(seg["near_ties"]).astype(np.int64).copy()
            if seg.get("best_state") is not None:
                self.best_state = np.array(seg["best_state"], dtype=np.uint8)
        else:
            if not np.array_equal(e0, self.energy):
                bad = int(np.flatnonzero(e0 != self.energy)[0])
                raise ValueError(f"chain {bad}: the segment starts at energy {int(e0[bad])}, the checkpoint stands at {int(self.energy[bad])}")
            lower = sbest < self.best_energy  # strictly: the first index of the minimum stays where it is on a tie
            self.best_energy = np.where(lower, sbest, self.best_energy)
            self.steps_to_best = np.where(lower, self.step + sstb, self.steps_to_best)
            if seg.get("best_state") is not None and self.best_state is not None:
                self.best_state = np.where(lower[:, None], np.asarray(seg["best_state"], dtype=np.uint8), self.best_state)
            self.n_accepted = self.n_accepted + np.asarray(seg["n_accepted"]).astype(np.int64)
            # a checkpoint without the count (saved by an earlier version, or a segment that lacked it) stays without: a sum of the later
            # segments alone would pass for the run's
            self.near_ties = None if self.near_ties is None or seg.get("near_ties") is None else self.near_ties + np.asarray(seg["near_ties"]).astype(np.int64)
        if seg.get("stream_words") is not None:
            self.stream_words = self.stream_words + np.asarray(seg["stream_words"]).astype(np.uint64)
        self.energy = np.asarray(seg["final_energy"]).astype(np.int64).copy()
        if seg.get("final_state") is not None:
            self.state = np.array(seg["final_state"], dtype=np.uint8)
        if seg.get("stream_state") is not None:
            self.stream_state = np.array(seg["stream_state"], dtype=np.uint32)
        self.step += seg_steps
        return self

    def save(self, path):
        """One .npz (no pickled objects): the per-chain arrays and a JSON record of what defines the run."""
        meta = {"format": FORMAT, "N": self.N, "mode": self.mode, "Q": self.Q, "schedule_params": self.schedule_params,
                "schedule_sets": self.schedule_sets, "chains_per_set": self.chains_per_set, "schedule_steps": self.schedule_steps,
                "trace": self.trace, "step": self.step}
        arrays = {k: getattr(self, k) for k in _PER_CHAIN if getattr(self, k) is not None}
        with open(path, "wb") as f:
            np.savez(f, meta=np.array(json.dumps(meta)), seeds=self.seeds, **arrays)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            meta = json.loads(str(z["meta"][()]))
            if meta.get("format") != FORMAT:
                raise ValueError(f"{path}: not a checkpoint of format {FORMAT}")
            c = cls(meta["N"], meta["mode"], meta["schedule_steps"], z["seeds"], schedule_params=meta["schedule_params"],
                    schedule_sets=meta["schedule_sets"], chains_per_set=meta["chains_per_set"], Q=meta["Q"], trace=meta["trace"])
            c.step = int(meta["step"])
            for k in _PER_CHAIN:
                if k in z.files:
                    setattr(c, k, z[k])
        return c
