"""The per-pair responsibility rows' ABI and keywords (no GPU needed): gw_step_out grew by exactly
one trailing pointer (fear_row), every earlier field kept its offset, the ctypes default is NULL,
and the Python entry points accept the opt-in keywords with their defaults off."""
import ctypes as C
import inspect

from marlnav import _lib


def test_step_out_grew_by_one_trailing_pointer():
    assert _lib.STEP_OUT_FIELDS[-1] == "fear_row"
    earlier = _lib.STEP_OUT_FIELDS[:-1]
    assert "fear_row" not in earlier

    class Before(C.Structure):  # the struct without its last field
        _fields_ = [(n, C.c_void_p) for n in earlier]

    assert C.sizeof(_lib.GwStepOut) == C.sizeof(Before) + C.sizeof(C.c_void_p)
    for n in earlier:
        assert getattr(_lib.GwStepOut, n).offset == getattr(Before, n).offset, n
    assert _lib.GwStepOut.fear_row.offset == C.sizeof(Before)


def test_fear_row_defaults_to_null():
    assert _lib.GwStepOut().fear_row is None
    # positional construction from the earlier fields alone (an older caller) leaves it NULL
    so = _lib.GwStepOut(*[None] * (len(_lib.STEP_OUT_FIELDS) - 1))
    assert so.fear_row is None


def test_accum_entry_point_is_declared():
    assert "gw_fear_row_accum" in _lib.EXPORTS
    lib = C.CDLL(_lib.build())
    assert hasattr(lib, "gw_fear_row_accum")


def test_keywords_exist_and_default_off():
    from marlnav.evaluate import evaluate
    from marlnav.rollout import Rollout
    from marlnav.vec_env import StepResult, VecGridEnv
    assert inspect.signature(VecGridEnv.__init__).parameters["fear_rows"].default is False
    assert inspect.signature(Rollout.__init__).parameters["resp_matrix"].default is False
    assert inspect.signature(evaluate).parameters["resp_matrix"].default is False
    f = {x.name: x for x in __import__("dataclasses").fields(StepResult)}
    assert f["fear_row"].default is None
