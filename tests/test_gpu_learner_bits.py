"""Both MADDPG learners (csrc/maddpg_dense.hip: gw_maddpg_critic_grads / gw_maddpg_actor_grads;
csrc/maddpg_desc.hip: gw_maddpg_desc_update[_img]) bit for bit against SHA-256 digests of what the
library computed BEFORE its sources were restructured (tests/golden/learner_bits.json).

tests/test_gpu_learner_shapes.py bounds the learners against float64; a restructuring that is meant
to change no bit is held to more: every output of every case below must keep its bits.

Dense: every case of tests/_learner_cases.DENSE (inputs and weight perturbation drawn on the CPU),
once with the Gumbel uniforms given and once with the in-kernel Philox draws: the critic phase, the
critic's Adam step (lr 1e-3, so the actor phase sees a stepped critic), the actor phase.  Digested:
every gradient tensor of both networks, both losses, ``probs`` and the action slots of ``x_next``.

Descriptor: every (scenario, B) of test_gpu_learner_shapes.DESC with its setup (64 envs, 7 steps,
the rollout acting through the torch actor), two learn_desc updates with one env step between them,
once without the actor env and once with it (gw_maddpg_desc_update_img).  Digested after each
update: the four flat parameter buffers, both optimizers' exp_avg / exp_avg_sq / grad, both losses,
the four c1 partial regions of the workspace, what desc_records returns and, with the actor env,
the fused actor's workspace past c1 (row slices, W2 / W3 images).  The ring (descriptors, probs,
reward, term, done) is digested before the first update under its own key: a ring that differs
fails as "inputs differ", not as a learner difference.  The rollout's torch actor gave the same ring
in both recordings (see ``record``), so the ring is filled as the shape sweep fills it.

``record(path)`` writes the digests (python tests/test_gpu_learner_bits.py <out.json>); it was run
twice against the old library and gave identical files."""
import ctypes as C_
import hashlib
import json
import os

import pytest
import torch

import _learner_cases as C
from test_gpu_learner_shapes import DESC, _desc_setup, _grads

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "learner_bits.json")
MODES = ("given", "philox")
RUNS = ("plain", "img")


def digest(named) -> str:
    """SHA-256 over (name, dtype, shape, bytes) of every tensor, in the order given."""
    h = hashlib.sha256()
    for name, t in named:
        t = t.detach().contiguous().cpu()
        h.update(f"{name}|{t.dtype}|{tuple(t.shape)}|".encode())
        h.update(t.view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def dense_digests(i, mode) -> dict:
    from marlnav import _lib
    from marlnav.maddpg import _mlp_spec
    c = C.dense_case(i)
    K, H, W, B, seed = c["K"], c["H"], c["W"], c["B"], c["seed"]
    m = C.make_learner(K, H, W, B, seed, "cuda", lr_critic=C.LR, capturable=True)
    assert m.fused
    C.perturb(m, seed)
    st, ac, rw, ns, dn, un, uc = [t.cuda() for t in c["batch"]]
    if mode == "philox":
        un = uc = None
    D = K * H * W
    x = m._critic_in(st, ac).contiguous()
    xn = m._critic_in(ns, torch.zeros_like(ac)).contiguous()
    ctx = m._learn_critic(st, ac, rw, ns, dn, un, (x, xn))
    assert ctx.get("fused")
    torch.cuda.synchronize()
    out = {"critic_grads": digest(zip(C.R.GRAD_NAMES, _grads(m.critics))),
           "critic_loss": digest([("loss", ctx["critic_loss"])]),
           "a_next": digest([("slots", ctx["x_next"][:, D:])])}
    m.opt_critic.step(advanced=True)
    probs = torch.full((K, B, 9), float("nan"), device=m.device)
    loss = torch.empty((K,), dtype=torch.float32, device=m.device)
    u = uc.to(torch.float32).contiguous() if uc is not None else None
    batch = m._fused_batch(ctx["x"], ctx["x_next"], ctx["r"], ctx["d"], u)
    a, cr, ag = _mlp_spec(m.actors.net), _mlp_spec(m.critics), _mlp_spec(m.actors.net, grad=True)
    _lib.check(_lib.load().gw_maddpg_actor_grads(C_.byref(a), C_.byref(cr), C_.byref(ag), C_.byref(batch),
                                                 m._fused_ws(B).data_ptr(), loss.data_ptr(), probs.data_ptr(),
                                                 m._count_ptr(m.opt_actor),
                                                 torch.cuda.current_stream(m.device).cuda_stream),
               "gw_maddpg_actor_grads")
    torch.cuda.synchronize()
    out.update({"actor_grads": digest(zip(C.R.GRAD_NAMES, _grads(m.actors.net))),
                "actor_loss": digest([("loss", loss)]), "probs": digest([("probs", probs)])})
    return out


def _cparts(m, rp):
    """The four c1 partial regions of the descriptor workspace (csrc dws_layout's order)."""
    ws, K, B = m._desc_setup(rp)["ws"], m.K, m.batch_size
    r4 = lambda n: (n + 3) // 4 * 4  # noqa: E731
    npm, NG = 9, (m.H * m.W + 63) // 64
    o = r4(2 * B) + 2 * r4(2 * K * B * npm) + r4(2 * K * B) + 2 * r4(B * 9 * K) + r4(2 * K * B * 9) + r4(K * B * 9) + \
        2 * r4(K * B) + 8 * r4(K * B * 128) + r4(K * B * 9) + r4(K * B)
    out = []
    for j, n in enumerate((K * NG * 128, K * NG * 128, K * K * NG * 128, K * K * NG * 128)):
        out.append((f"cpart{j}", ws[o:o + n]))
        o += r4(n)
    assert o + 8 == ws.numel()  # snap and adsc follow
    return out


def desc_digests(sid, B, run) -> dict:
    sc, env, m, m3, ro = _desc_setup(sid, B)
    try:
        rp = ro.replay
        assert m.desc_capable(rp)
        torch.cuda.synchronize()
        out = {"inputs": digest([(n, getattr(rp, n)) for n in ("desc", "probs", "reward", "term", "done")])}
        actor_env = None
        if run == "img":
            m.actors.ensure_workspace(env)
            actor_env = env
            assert m._actor_images(env) is not None
        for upd in (1, 2):
            if upd == 2:
                ro.step()
                ro.fence()
            la, lc = m.learn_desc(rp, actor_env=actor_env)
            rec = m.desc_records(rp)
            torch.cuda.synchronize()
            d = {"params": digest([(n, net.flat_params()) for n, net in
                                   (("actor", m.actors.net), ("actor_target", m.actor_targets.net), ("critic", m.critics),
                                    ("critic_target", m.critic_targets))]),
                 "optim": digest([(f"{n}.{f}", t) for n, o in (("actor", m.opt_actor), ("critic", m.opt_critic))
                                  for f, t in (("exp_avg", o.m), ("exp_avg_sq", o.v), ("grad", o.flat.grad))]),
                 "losses": digest([("actor", la), ("critic", lc)]),
                 "cpart": digest(_cparts(m, rp)),
                 "records": digest(sorted(rec.items()))}
            if run == "img":
                d["actor_ws"] = digest([("ws", m.actors._fast["ws"][m.K * 128:])])
            out[f"update{upd}"] = d
        return out
    finally:
        env.close()


def record(path):
    """Everything this file compares, as {"_recorded": note, "dense": ..., "desc": ...}."""
    rec = {"_recorded": "SHA-256 digests recorded on an MI355X from the library of the commit BEFORE "
                        "csrc/maddpg_ops.hip was split into maddpg_dense.hip / maddpg_desc.hip, never from the "
                        "restructured code; two recordings gave identical files",
           "dense": {C.DENSE_IDS[i]: {mode: dense_digests(i, mode) for mode in MODES} for i in range(len(C.DENSE))},
           "desc": {sid: {run: desc_digests(sid, B, run) for run in RUNS} for sid, B in DESC}}
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("i", range(len(C.DENSE)), ids=C.DENSE_IDS)
def test_dense_learner_bits(i, mode):
    want = _golden()["dense"][C.DENSE_IDS[i]][mode]
    got = dense_digests(i, mode)
    assert set(got) == set(want)
    assert not [n for n in sorted(want) if got[n] != want[n]], "learner differs"


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("sid,B", DESC, ids=[d[0] for d in DESC])
def test_desc_learner_bits(sid, B, run):
    want = _golden()["desc"][sid][run]
    got = desc_digests(sid, B, run)
    assert got["inputs"] == want["inputs"], "inputs differ"
    assert set(got) == set(want)
    bad = [f"{u}.{n}" for u in ("update1", "update2") for n in sorted(want[u]) if got[u].get(n) != want[u][n]]
    assert not bad, f"learner differs: {bad}"


if __name__ == "__main__":
    import sys
    record(sys.argv[1])
