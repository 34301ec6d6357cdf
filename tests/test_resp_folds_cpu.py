"""The shared responsibility folds (marlnav/resp_folds.py) without a device: which folds the keywords arm, and
that every fold reads its own slice of the concatenated float64 vector back, for every subset of the keywords.

The env is a stand-in (sizes, a device and an ``out`` dict of zero tensors): constructing a fold and reducing
it touch no library.  The all-reduce is a two-rank one of equal ranks: every value doubles."""
import itertools
from types import SimpleNamespace

import pytest
import torch

import marlnav
from marlnav import resp_folds as RF

K, N, H, W, E, R = 2, 4, 5, 7, 6, 2
KEYWORDS = ("resp_matrix", "fear_regret", "feal", "resp_full", "resp_map", "resp_footprint")
OUT_KEYS = ("fear_row", "fear_alt", "fear", "feal", "resp_full", "resp_valid", "actions", "crash_bits")


def _env(without=()):
    out = {k: torch.zeros(1) for k in OUT_KEYS if k not in without}
    return SimpleNamespace(K=K, N=N, H=H, W=W, E=E, device=torch.device("cpu"), out=out)


def _kwargs(subset):
    return {k: (R if k == "resp_footprint" else True) for k in subset}


SUBSETS = [s for n in range(len(KEYWORDS) + 1) for s in itertools.combinations(KEYWORDS, n)]


@pytest.mark.parametrize("subset", SUBSETS, ids=lambda s: "+".join(s) or "none")
def test_armed_list_and_readback(subset):
    folds, cells = RF.build_folds(_env(), "Rollout", **_kwargs(subset))
    # the rules: launch order, map arms full, map and footprint share one [N, E] int32 cells buffer
    want = [(RF.RowFold, "resp_matrix" in subset), (RF.RegretFold, "fear_regret" in subset),
            (RF.FealFold, "feal" in subset), (RF.RowFold, "resp_full" in subset or "resp_map" in subset),
            (RF.MapFold, "resp_map" in subset), (RF.FootprintFold, "resp_footprint" in subset)]
    assert [type(f) for f in folds] == [cls for cls, on in want if on]
    assert [f.key for f in folds if isinstance(f, RF.RowFold)] == \
        [k for k, on in (("resp", want[0][1]), ("resp_full", want[3][1])) if on]
    binned = [f for f in folds if isinstance(f, (RF.MapFold, RF.FootprintFold))]
    assert (cells is not None) == bool(binned)
    if binned:
        assert tuple(cells.shape) == (N, E) and cells.dtype == torch.int32
        assert all(f.cells is cells for f in binned)

    # distinct known values in every buffer of every fold
    base = 1
    for f in folds:
        for name, t in vars(f).items():
            if isinstance(t, torch.Tensor) and t is not cells:
                t.copy_((torch.arange(t.numel()) + base).reshape(t.shape))
                base += t.numel()
    before = [{n: t.clone() for n, t in vars(f).items() if isinstance(t, torch.Tensor)} for f in folds]

    parts, widths = RF.fold_parts(folds)
    assert all(p.dtype == torch.float64 and p.dim() == 1 for p in parts)
    assert sum(widths) == sum(p.numel() for p in parts)
    if not subset:  # nothing armed: nothing to reduce, nothing to report
        assert (folds, cells, parts, widths) == ([], None, [], [])
        assert RF.fold_results(folds, widths, None) == {}
        return
    flat = torch.cat(parts) * 2 if parts else None
    reduced = []

    def all_reduce(t):
        reduced.append(tuple(t.shape))
        t.mul_(2)

    res = RF.fold_results(folds, widths, flat, all_reduce)
    for f, b in zip(folds, before):  # the all-reduce works on copies: the running totals are untouched
        assert all(torch.equal(getattr(f, n), t) for n, t in b.items())

    want_keys, by_cls = [], {(type(f), getattr(f, "key", None)): b for f, b in zip(folds, before)}

    def same(key, t, shape, dtype=torch.float64):
        want_keys.append(key)
        assert res[key].dtype == dtype and tuple(res[key].shape) == shape and res[key].device.type == "cpu", key
        assert torch.equal(res[key], t.reshape(shape)), key

    def count(key, v):
        want_keys.append(key)
        assert type(res[key]) is int and res[key] == int(v), key

    for key, rows in (("resp", K), ("resp_full", N)):
        b = by_cls.get((RF.RowFold, key))
        if b is not None:
            same(key, 2 * b["total"], (rows, N))
            count(key + "_steps", b["steps"])  # this rank's steps: not summed over the ranks
    b = by_cls.get((RF.RegretFold, None))
    if b is not None:
        same("fear_regret", 2 * b["total"][:, 0], (K,))
        same("fear_best", 2 * b["total"][:, 1], (K,))
        count("fear_regret_steps", b["steps"])
    b = by_cls.get((RF.FealFold, None))
    if b is not None:
        same("feal_sum", 2 * b["total"], (N,))
        count("feal_envs", 2 * b["cnt"][1])  # rides in the float64 vector
        count("feal_steps", b["cnt"][0])
    want_reduced = []
    b = by_cls.get((RF.MapFold, None))
    if b is not None:
        same("resp_map_counts", 2 * b["counts"], (2, H * W, 10, 10), torch.int64)
        same("resp_map_visits", 2 * b["visits"], (H * W,), torch.int64)
        same("resp_map", marlnav.resp_map_from_counts(2 * b["counts"])[0], (2, H, W))
        want_reduced += [(2, H * W, 10, 10), (H * W,)]
    b = by_cls.get((RF.FootprintFold, None))
    if b is not None:
        O = (2 * R + 1) ** 2 + 1
        same("resp_footprint_counts", 2 * b["counts"], (2, 9, O, 10, 10), torch.int64)
        same("resp_footprint_visits", 2 * b["visits"], (9,), torch.int64)
        same("resp_footprint", marlnav.resp_footprint_from_counts(2 * b["counts"])[0], (2, 9, O))
        want_reduced += [(2, 9, O, 10, 10), (9,)]
    assert sorted(res) == sorted(want_keys)
    assert reduced == want_reduced  # the integer collectives: map counts, visits, then the footprint's


@pytest.mark.parametrize("who", ["Rollout", "evaluate"])
def test_missing_env_output_names_the_caller_and_the_keyword(who):
    for kw, missing, text in (
            (dict(resp_matrix=True), ("fear_row",), "(resp_matrix=True) needs VecGridEnv(fear_rows=True)"),
            (dict(fear_regret=True), ("fear_alt",), "(fear_regret=True) needs VecGridEnv(fear_alt=True)"),
            (dict(feal=True), ("feal",), "(feal=True) needs VecGridEnv(feal=True)"),
            (dict(resp_full=True), ("resp_full",), "(resp_full=True) needs VecGridEnv(fear_full=True)"),
            # the map is checked before the full matrix it arms: the text names the keyword the caller gave
            (dict(resp_map=True), ("resp_valid", "resp_full"), "(resp_map=True) needs VecGridEnv(fear_full=True)"),
            (dict(resp_footprint=R), ("resp_valid",), "(resp_footprint=R) needs VecGridEnv(fear_full=True)"),
            (dict(resp_footprint=R), ("actions",), "(resp_footprint=R) needs VecGridEnv(debug=True) (the step's "
                                                   "actions and crash_bits)"),
            (dict(resp_footprint=R), ("crash_bits",), "(resp_footprint=R) needs VecGridEnv(debug=True)")):
        with pytest.raises(ValueError) as e:
            RF.build_folds(_env(without=missing), who, **kw)
        assert str(e.value).startswith(who + text), str(e.value)


def test_footprint_radius_range():
    for bad in (0, 16, -3):
        with pytest.raises(ValueError, match=r"Rollout\(resp_footprint=R\): R in 1\.\.15"):
            RF.build_folds(_env(), "Rollout", resp_footprint=bad)
    for ok in (1, 15):
        (f,), _ = RF.build_folds(_env(), "evaluate", resp_footprint=ok)
        assert tuple(f.counts.shape) == (2, 9, (2 * ok + 1) ** 2 + 1, 10, 10)


def test_shield_argument_check():
    from marlnav.rollout import Rollout
    RF.check_shield_args("unilateral", True)
    RF.check_shield_args("joint", False)
    with pytest.raises(ValueError, match=r"evaluate\(shield_crash=True\) with shield_mode=\"joint\""):
        RF.check_shield_args("joint", True, "evaluate")
    with pytest.raises(ValueError, match=r"Rollout\(shield_mode=\.\.\.\)"):
        RF.check_shield_args("sideways", False)
    with pytest.raises(ValueError, match=r"Rollout\(shield_crash=True\)"):
        Rollout.check_shield_args("joint", True)  # the static method is the module's check
    with pytest.raises(ValueError, match="shield_crash"):  # the Shield refuses before it allocates anything
        RF.Shield(SimpleNamespace(), 0.0, "joint", crash=True)
