"""The descriptor-only window ring on the CPU: the window rule gw_replay_gather_desc_patch expands
(include/rollout_ops.h; restated in tests/_desc_patch.py) against crops of the oracle-pinned full
observations, the kernel's one multiply-by-reciprocal over the whole range it runs on, and the documented
error of the CPU path (the product has no CPU fallback)."""
import os
import types

import numpy as np
import pytest
import torch

import _desc_patch as DP
import _shapes as SH

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "marl-responsible-nav_amd", "csrc")


@pytest.mark.parametrize("sid,P", [("7x9_n3_k3", 5), ("13x3_n3_k1", 9), ("2x2_n4_k2", 2), ("1x8_n2_k1", 3)])
def test_window_rule_equals_crops_of_the_oracle_obs(sid, P):
    """An oracle rollout at the sweep's parameters: after the reset and every step, the window built from what a
    descriptor half holds (the agents' cells, the apple bits, the reset flag) equals the crop of the oracle's
    full obs around agent k's cell, padded with -1: the step obs, the reset obs of the envs that ended
    (auto-reset) and their terminal obs.  The terminal obs' apple bits are not in the oracle's step record;
    bit k is read from the terminal obs' value under the apple cell (>= 9 exactly when present), which leaves
    the window's geometry, the override order and every agent value to the rule under test."""
    from oracle import oracle as O
    sc, E = SH.scenario(sid), SH.SWEEP["E"]
    H, W, N, K = sc.H, sc.W, sc.N, sc.K
    base = np.where(np.asarray(sc.region).reshape(H, W) != 0, 0.0, -1.0).astype(np.float32)
    orc = O.OracleEnvs(sc, E, fear=True, fear_weight=-5.0, max_steps=SH.SWEEP["max_steps"], seed=SH.SWEEP["seed"],
                       reset=False)
    obs = np.zeros((K, E, H * W), np.float32)
    fin = np.full((K, E, H * W), np.nan, np.float32)
    orc.reset_all(obs=obs)
    outs = (O.StepOut * E)()
    all_bits = (1 << K) - 1

    def check(cells, bits, reset, full, k, what):
        w = DP.window(cells, bits, reset, k, P, base, sc.apples)
        np.testing.assert_array_equal(w, DP.crop(full.reshape(H, W), cells[k], P), err_msg=what)

    pos = orc.positions()
    for e in range(E):
        for k in range(K):
            check(pos[e], all_bits, True, obs[k, e], k, f"reset e{e} k{k}")
    n_done = n_overhang = 0
    for t in range(SH.SWEEP["steps"]):
        orc.vec_step(None, obs=obs, outs=outs, final_obs=fin)
        pos = orc.positions()
        for e in range(E):
            done = bool(outs[e].done)
            n_done += done
            bits = all_bits if done else int(orc.envs[e].apples)
            for k in range(K):
                check(pos[e], bits, done, obs[k, e], k, f"step {t} e{e} k{k}")
                cr, cc = divmod(int(pos[e][k]), W)
                n_overhang += cr - P // 2 < 0 or cc - P // 2 < 0 or cr - P // 2 + P > H or cc - P // 2 + P > W
            if done:
                fpos = np.array(list(outs[e].final_pos)[:N])
                fbits = sum(int(fin[k, e, sc.apples[k]] >= 9.0) << k for k in range(K))
                for k in range(K):
                    check(fpos, fbits, False, fin[k, e], k, f"terminal {t} e{e} k{k}")
    assert n_done > 0 and n_overhang > 0


def test_quotient_by_P_is_exact_for_every_window_cell():
    """replay_gather_desc_patch_kernel's one multiply-high: wr = __umulhi(i, m_p) with m_p = min(2^32 - 1,
    ceil(2^32 / P)) for every window cell i < P * P and every P gw_obs_patch takes (1 .. 129).  With m = (2^32 +
    r) / P, r < P, the product overshoots i / P by i r / (P 2^32) < 1 / P while i r < 2^32; i < 16,641 and r < 129
    give i r < 2^22.  P == 1 is the one clamped multiplier (2^32 does not fit); its only cell is i == 0, whose
    quotient is 0 under any multiplier.  Checked exhaustively rather than trusted.  The divisions by W run
    once per patched cell and are plain integer divisions."""
    s32 = np.uint64(32)
    for P in range(1, DP.MAXP + 1):
        i = np.arange(P * P, dtype=np.uint64)
        m = DP.magic(P)
        assert (m == np.uint64(0xFFFFFFFF)) == (P == 1)
        np.testing.assert_array_equal((i * m) >> s32, i // np.uint64(P), err_msg=str(P))
    # beyond the range it runs on the clamped multiplier would be wrong: P == 1 relies on i == 0 alone
    assert (np.uint64(1) * DP.magic(1)) >> s32 != np.uint64(1)


def test_descriptor_only_ring_raises_on_the_cpu():
    from marlnav.rollout import ReplayRing
    env = types.SimpleNamespace(K=2, E=8, H=32, W=32, device=torch.device("cpu"), obs_dtype=torch.float32, handle=None)
    with pytest.raises(ValueError, match="no CPU path"):
        ReplayRing(env, 4, patch=11, desc="only")
    with pytest.raises(ValueError, match="patch > 0"):
        ReplayRing(env, 4, patch=0, desc="only")
    with pytest.raises(ValueError, match='"only"'):
        ReplayRing(env, 4, patch=11, desc="all")
    ring = ReplayRing(env, 4, patch=11, desc=True)  # unchanged: ignored with patch, the dense window ring
    assert ring.desc is None and tuple(ring.obs.shape) == (4, 2, 8, 11, 11) and not ring.desc_only


def test_new_source_is_listed_and_reads_no_environment():
    """The release library's sources include the new translation unit and its header (the stamp and the
    objects' hashes cover them), and the new source reads no environment variable (tests/test_lib_cpu.py's
    release-library check stays as it is)."""
    from marlnav import _lib
    names = [os.path.basename(p) for p in _lib.HIP_SOURCES]
    assert "replay_patch.hip" in names
    assert os.path.join(CSRC, "desc_rows.h") in _lib.SOURCES
    assert "gw_replay_gather_desc_patch" in _lib.EXPORTS
    for f in ("replay_patch.hip", "desc_rows.h"):
        with open(os.path.join(CSRC, f)) as fh:
            assert "getenv" not in fh.read(), f
    with open(os.path.join(CSRC, "rollout_ops.hip")) as fh:
        text = fh.read()
    assert "desc_patches(const DescSrc" not in text and '#include "desc_rows.h"' in text  # one statement of the encoding
