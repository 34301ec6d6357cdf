"""The dense fused MADDPG update (csrc/maddpg_dense.hip: gw_maddpg_critic_grads / gw_maddpg_actor_grads)
against a float64 restatement of the update (tests/_maddpg_ref64.py, tied to the per-agent loop in
tests/test_maddpg_ref64_cpu.py) at the shapes where the kernels branch (tests/_learner_cases.py):
D % 4, D % 16, D / K*D / K*D + 9K modulo the 64-input chunks, more than RED_PRE chunks, row tiles
with a 16-row tail, K up to GW_MAX_AGENTS.

Each case builds a fused learner and its f32 autograd twin with targets apart from the online
networks, non-trivial LayerNorm affines and a critic learning rate of 0 (so the actor phase sees the
initial critic and the whole reference is known before anything runs on the GPU), on a batch with
forced rows (all dones 1, all dones 0, a reward of 1e6 + 1/3, Gumbel uniforms of exactly 0 and of
the largest float below 1).  Rows with a ReLU input within EDGE of zero in the float64 reference are
replaced by a copy of a clean row (at most B / 8, checked on the CPU).

Per tensor: every gradient tensor and both losses of the fused update within 1e-5 relative L2 of
float64; the target actions and the actor's fresh probabilities (gw_maddpg_actor_grads' ``probs``
output, which no Python path reads) within 2e-6.
Every stacked tensor and both losses are judged agent by agent (the worst agent counts): the agent
that holds the 1e6 reward has gradients 1e5 times the others' and would hide them in a norm over
the stack.
Per block: the W1 gradients cut into grads_kernel's 16-input blocks and into l1_kernel's 64-input
chunks, the W2 gradients into their 16-row blocks; a block's error is ||got - ref|| / (rms(ref
tensor) sqrt(block elements)), and must stay within 4 x the largest block error of the f32 autograd
composition against the same float64 reference (floor 1e-6): both are f32 sums of the same terms in
different orders.  Negative controls on one small case show that the checks bite.

The descriptor learner (gw_maddpg_desc_update) runs on the open maps of tests/_shapes.py (HW of 4, 8,
12, 25, 39, 40 and a 6 x 6 map with N = K = 8) for two updates with an env step between them; see
test_desc_learner_matches_float64.
"""
import ctypes as C_
import json

import pytest
import torch

import _learner_cases as C
import _maddpg_ref64 as R

pytestmark = pytest.mark.gpu

GRAD_TOL, PROB_TOL, BLOCK_FACTOR, BLOCK_FLOOR = 1e-5, 2e-6, 4.0, 1e-6


def _grads(net):
    return [p.grad.detach().clone() for p in (net.weights[0], net.biases[0], net.ln_w[0], net.ln_b[0], net.weights[1],
                                              net.biases[1], net.ln_w[1], net.ln_b[1], net.weights[2], net.biases[2])]


def _rel(got, ref):
    """Relative L2 per agent (dim 0 of every stacked tensor), the worst agent's: the stacked tensor's
    norm would let the agent with the 1e6 reward hide the others."""
    K = ref.shape[0]
    d, r = (got.double() - ref).reshape(K, -1).norm(dim=1), ref.reshape(K, -1).norm(dim=1)
    return float((d / r.clamp_min(1e-300)).max())


def block_errors(got, ref, blk):
    """got / ref [K, rows, 128] -> [K, ceil(rows / blk)]: per block of ``blk`` rows,
    ||got - ref|| / (rms(ref[k]) sqrt(block elements)), agent k's own tensor as the scale."""
    rms = ref.pow(2).mean(dim=(1, 2)).sqrt()
    d = (got.double() - ref) ** 2
    out = [(d[:, r0:r0 + blk].sum(dim=(1, 2)) / d[:, r0:r0 + blk][0].numel()).sqrt() / rms
           for r0 in range(0, ref.shape[1], blk)]
    return torch.stack(out, 1)


# (name, network, index in GRAD_NAMES, block rows)
BLOCKS = [("critic.w1/16", "critic", 0, 16), ("critic.w1/64", "critic", 0, 64), ("critic.w2/16", "critic", 4, 16),
          ("actor.w1/16", "actor", 0, 16), ("actor.w1/64", "actor", 0, 64), ("actor.w2/16", "actor", 4, 16)]


def tensors(res) -> dict:
    """name -> tensor of everything the per-tensor bound covers."""
    out = {}
    for net in ("critic", "actor"):
        for n, g in zip(R.GRAD_NAMES, res[net]):
            out[f"{net}.{n}"] = g
        out[f"{net}.loss"] = res[f"{net}_loss"]
    return out


def tensor_errors(got, ref) -> dict:
    """Everything agent by agent, the worst agent's figure.  A critic loss is a sum of squares, so its own
    value is its scale.  An actor loss -mean_b Q can cancel to nearly nothing (K = 8, B = 32: 1.3e-5 of
    its own value in the fused update and in the autograd composition alike), so its error is taken
    relative to mean_b |Q| of the agent, the size of the terms it sums."""
    tg, tr = tensors(got), tensors(ref)
    out = {n: _rel(tg[n], tr[n]) for n in tr if n != "actor.loss"}
    out["actor.loss"] = float(((tg["actor.loss"].double() - tr["actor.loss"]).abs() / ref["actor_q_abs"]).max())
    return out


def block_report(got, auto, ref) -> dict:
    """name -> (fused's block errors [K, nb], the bound from the autograd composition's)."""
    out = {}
    for name, net, j, blk in BLOCKS:
        e_auto = block_errors(auto[net][j], ref[net][j], blk)
        out[name] = (block_errors(got[net][j], ref[net][j], blk), max(BLOCK_FACTOR * float(e_auto.max()), BLOCK_FLOOR),
                     float(e_auto.max()))
    return out


def failures(got, auto, ref) -> dict:
    """What misses its bound: tensor names, block positions (k, block) per block check, and the
    probability tensors."""
    f = {"tensors": sorted(n for n, e in tensor_errors(got, ref).items() if not e < GRAD_TOL), "blocks": {},
         "probs": [n for n in ("a_next", "probs")
                   if got.get(n) is not None and not float((got[n].double() - ref[n]).abs().max()) <= PROB_TOL]}
    for name, (e, bound, _) in block_report(got, auto, ref).items():
        bad = (~(e <= bound)).nonzero().tolist()
        if bad:
            f["blocks"][name] = [tuple(b) for b in bad]
    return f


def _ref_result(c, a, device):
    f = lambda t: t.to(device)  # noqa: E731
    return {"critic": [f(g) for g in c["grads"]], "actor": [f(g) for g in a["grads"]], "critic_loss": f(c["loss"]),
            "actor_loss": f(a["loss"]), "actor_q_abs": f(a["q_abs"]), "a_next": f(c["a_next"]), "probs": f(a["probs"])}


def _fused_probs(m, ctx, uc):
    """gw_maddpg_actor_grads once more with its ``probs`` output given: the fresh probabilities
    [K, B, 9]; the gradients and the loss it rewrites must be the first call's bits."""
    from marlnav import _lib
    from marlnav.maddpg import _mlp_spec
    K, B = m.K, ctx["B"]
    before, loss0 = _grads(m.actors.net), ctx["actor_loss"].clone()
    probs = torch.full((K, B, 9), float("nan"), device=m.device)
    loss = torch.empty((K,), dtype=torch.float32, device=m.device)
    u = uc.to(torch.float32).contiguous()
    batch = m._fused_batch(ctx["x"], ctx["x_next"], ctx["r"], ctx["d"], u)
    a, c, ag = _mlp_spec(m.actors.net), _mlp_spec(m.critics), _mlp_spec(m.actors.net, grad=True)
    _lib.check(_lib.load().gw_maddpg_actor_grads(C_.byref(a), C_.byref(c), C_.byref(ag), C_.byref(batch),
                                                 m._fused_ws(B).data_ptr(), loss.data_ptr(), probs.data_ptr(), None,
                                                 torch.cuda.current_stream(m.device).cuda_stream),
               "gw_maddpg_actor_grads")
    torch.cuda.synchronize()
    assert torch.equal(loss, loss0)
    for g0, g1 in zip(before, _grads(m.actors.net)):
        assert torch.equal(g0, g1)
    return probs


def _block_record(blocks) -> dict:
    return {n: {"fused": float("%.2e" % float(e.max())), "autograd": float("%.2e" % ea),
                "ratio": float("%.3g" % (float(e.max()) / max(ea, BLOCK_FLOOR / BLOCK_FACTOR)))}
            for n, (e, _, ea) in blocks.items()}


_RUNS = {}


def run_dense(i):
    """Case i on the GPU, once per session: (fused, f32 autograd composition, float64 reference)."""
    if i in _RUNS:
        return _RUNS[i]
    from marlnav.maddpg import gumbel_softmax
    c = C.dense_case(i)
    K, H, W, B, seed = c["K"], c["H"], c["W"], c["B"], c["seed"]
    ms = [C.make_learner(K, H, W, B, seed, "cuda", capturable=True) for _ in range(2)]
    assert ms[0].fused
    ms[1].fused = False
    for m in ms:
        C.perturb(m, seed)
        for name, net in (("actor", m.actors.net), ("actor_target", m.actor_targets.net), ("critic", m.critics),
                          ("critic_target", m.critic_targets)):  # the weights the CPU reference was computed for
            for t, t64 in zip(R.leaves(R.net64(net, "cpu")), R.leaves(c["P"][name])):
                assert torch.equal(t, t64), name
    st, ac, rw, ns, dn, un, uc = [t.cuda() for t in c["batch"]]
    D = K * H * W
    res = []
    for m in ms:
        x = m._critic_in(st, ac).contiguous()
        xn = m._critic_in(ns, torch.zeros_like(ac)).contiguous()
        before = m.critics.flat_params().detach().clone()
        ctx = m._learn_critic(st, ac, rw, ns, dn, un, (x, xn))
        gc = _grads(m.critics)
        m._learn_actor(ctx, uc)
        torch.cuda.synchronize()
        assert torch.equal(m.critics.flat_params().detach(), before)  # lr_critic = 0: the initial critic
        if m.fused:
            assert ctx.get("fused")
            probs = _fused_probs(m, ctx, uc)
        else:
            with torch.no_grad():
                probs = gumbel_softmax(m.actors(st), uc)
        res.append({"critic": gc, "actor": _grads(m.actors.net), "critic_loss": ctx["critic_loss"].clone(),
                    "actor_loss": ctx["actor_loss"].clone(),
                    "a_next": xn[:, D:].reshape(B, K, 9).permute(1, 0, 2).contiguous(), "probs": probs})
    _RUNS[i] = (res[0], res[1], _ref_result(c["critic"], c["actor"], "cuda"))
    return _RUNS[i]


@pytest.mark.parametrize("i", range(len(C.DENSE)), ids=C.DENSE_IDS)
def test_dense_fused_update_matches_float64(i):
    c = C.dense_case(i)
    assert c["edge_left"] == 0 and len(c["masked"]) <= c["B"] // 8
    got, auto, ref = run_dense(i)
    e_got, e_auto = tensor_errors(got, ref), tensor_errors(auto, ref)
    blocks = block_report(got, auto, ref)
    rec = {"case": C.DENSE_IDS[i], "masked": len(c["masked"]),
           "fused": {n: float("%.2e" % e) for n, e in e_got.items()},
           "autograd": {n: float("%.2e" % e) for n, e in e_auto.items()},
           "a_next": float((got["a_next"].double() - ref["a_next"]).abs().max()),
           "probs": float((got["probs"].double() - ref["probs"]).abs().max()), "blocks": _block_record(blocks)}
    print("REF64 " + json.dumps(rec))
    f = failures(got, auto, ref)
    assert not f["probs"], f
    assert not f["tensors"], (f, e_got)
    assert not f["blocks"], f


NEG = 2  # K = 3, 7 x 9, B = 144


def test_negative_control_one_w1_block_scaled():
    """One 16-input block of the critic's W1 gradient scaled by 1 + 1e-4 fails the 16-input block check
    for exactly that block.  The 64-input chunk that holds it and critic.w1's per-tensor bound may
    report it too (the same elements seen at a coarser grain); nothing else reports anything."""
    got, auto, ref = run_dense(NEG)
    assert failures(got, auto, ref) == {"tensors": [], "blocks": {}, "probs": []}
    k, blk = 1, 5
    bad = dict(got, critic=[g.clone() for g in got["critic"]])
    bad["critic"][0][k, 16 * blk:16 * (blk + 1)] *= 1.0 + 1e-4
    f = failures(bad, auto, ref)
    assert f["blocks"].get("critic.w1/16") == [(k, blk)], f
    # the 64-input chunk that holds the block may notice as well; no other tensor and no other block does
    assert set(f["blocks"]) <= {"critic.w1/16", "critic.w1/64"} and f["blocks"].get("critic.w1/64", [(k, blk // 4)]) == \
        [(k, blk // 4)], f
    assert f["probs"] == [] and set(f["tensors"]) <= {"critic.w1"}, f


def _reference_with(i, change):
    c = C.dense_case(i)
    P = {name: {k: [t.clone() for t in v] for k, v in net.items()} for name, net in c["P"].items()}
    change(P)
    return _ref_result(*C.reference(P, c["batch"]), "cuda")


def test_negative_control_online_critic_as_target():
    """A reference that evaluates the online critic where the update evaluates the target critic is
    told apart: the critic phase fails, the target actions and the actor phase (which never read
    the target critic) still pass."""
    got, auto, _ = run_dense(NEG)

    def change(P):
        P["critic_target"] = P["critic"]
    f = failures(got, auto, _reference_with(NEG, change))
    assert f["probs"] == [] and f["tensors"], f
    assert all(n.startswith("critic.") for n in f["tensors"]) and {"critic.w1", "critic.w2", "critic.w3", "critic.loss"} <= set(f["tensors"]), f
    assert all(n.startswith("critic.") for n in f["blocks"]), f


def test_negative_control_ln_b_dropped():
    """A reference without the LayerNorm biases is told apart in both phases."""
    got, auto, _ = run_dense(NEG)

    def change(P):
        for net in P.values():
            for t in net["lb"]:
                t.zero_()
    f = failures(got, auto, _reference_with(NEG, change))
    assert "critic.w1" in f["tensors"] and "actor.w1" in f["tensors"], f
    assert f["probs"] == ["a_next", "probs"], f


# ---- the descriptor learner -------------------------------------------------------------------------
# (scenario, B): the open maps of tests/_shapes.py and a 6 x 6 map whose N = K = 8 agents fill every patch
# slot of an obs and every decoder thread of the tails (tid < RB * 2 * K = 256)
DESC = [("1x8_n2_k1", 16), ("2x2_n4_k2", 48), ("3x4_n7_k7", 256), ("5x5_n6_k4", 48), ("13x3_n3_k1", 256),
        ("5x8_n5_k5", 16), ("open6x6_n8_k8", 48)]
DESC_E, DESC_CAP, DESC_STEPS, DESC_SEED = 64, 4, 7, 7


def _desc_setup(sid, B):
    """tests/test_gpu_desc_learner.py's _setup on an open map: E = 64, episodes capped at 4 steps so that
    the 7 stored transitions hold finished episodes and reset obs; targets apart and random LayerNorm
    affines before anything runs.  The rollout acts through the torch actor (fused = False): what is
    under test is the learner, and the ring's descriptors come from the step kernels either way."""
    import _shapes
    from marlnav.rollout import Rollout
    from marlnav.vec_env import VecGridEnv
    sc = _shapes.open_scenario(6, 6, 8, 8) if sid.startswith("open") else _shapes.scenario(sid)
    env = VecGridEnv(sc, num_envs=DESC_E, fear=True, fear_weight=-5.0, stats=True, seed=DESC_SEED, max_steps=DESC_CAP)
    ms = [C.make_learner(sc.K, sc.H, sc.W, B, 3, env.device, lr_critic=lr, capturable=True) for lr in (C.LR, 0.0)]
    C.perturb(ms[0], 3)
    ms[1].fused = False  # the f32 autograd composition; it takes the learner's weights before every update
    ro = Rollout(env, ms[0].actors, replay_slots=16, training=True, seed=4, fused=False, desc_ring=True)
    ro.reset()
    for _ in range(DESC_STEPS):
        ro.step()
    ro.fence()
    return sc, env, ms[0], ms[1], ro


def _nets(m):
    return (m.actors.net, m.actor_targets.net, m.critics, m.critic_targets)


def _desc_update(sc, m, m3, ro):
    """One learn_desc of m on the ring -> (got, the f32 composition on the same rows, float64 reference,
    facts about the sampled rows).  Edge rows (a ReLU input within EDGE of zero in float64) cannot be
    replaced, the kernel draws the sample: their exact float64 contribution (the reference minus the
    reference with those rows' loss weights zeroed) is subtracted from all three sides, so the
    comparison is scaled by the clean rows' gradient."""
    from test_gpu_desc_learner import _dense_batch
    rp, K, B = ro.replay, m.K, m.batch_size
    assert m.desc_capable(rp)
    P = R.params64(m, "cpu")
    with torch.no_grad():
        for dst, src in zip(_nets(m3), _nets(m)):
            dst.flat_params().copy_(src.flat_params())
    la, lc = m.learn_desc(rp)
    rec = m.desc_records(rp)
    torch.cuda.synchronize()
    got = {"critic": _grads(m.critics), "actor": _grads(m.actors.net), "critic_loss": lc.clone(), "actor_loss": la.clone(),
           "a_next": rec["a_next"].reshape(B, K, 9).permute(1, 0, 2).contiguous()}
    st, ac, rw, ns, dn = _dense_batch(rp, rec["idx"])
    # the f32 composition: the critic phase on the initial weights, the actor phase on the learner's stepped critic
    ctx = m3._learn_critic(st, ac, rw, ns, dn, rec["u_next"])
    auto = {"critic": _grads(m3.critics)}
    with torch.no_grad():
        m3.critics.flat_params().copy_(m.critics.flat_params())
    m3._learn_actor(ctx, rec["u_cur"])  # (its own critic step has learning rate 0)
    torch.cuda.synchronize()
    auto["actor"] = _grads(m3.actors.net)
    b = [t.cpu() for t in (st, ac, rw, ns, dn, rec["u_next"], rec["u_cur"])]
    after = R.net64(m.critics, "cpu")
    c, a = C.reference(P, b, critic_after=after)
    edge = R.edge_rows((c, a), C.EDGE)
    ref = _ref_result(c, a, "cuda")
    if edge.any():
        c2, a2 = C.reference(P, b, critic_after=after, row_w=(~edge).double())
        for net, full, clean in (("critic", c, c2), ("actor", a, a2)):
            for j in range(10):
                d = (full["grads"][j] - clean["grads"][j]).cuda()
                got[net][j], auto[net][j] = got[net][j].double() - d, auto[net][j].double() - d
                ref[net][j] = clean["grads"][j].cuda()
    tr, e = rec["idx"][:, 0].long(), rec["idx"][:, 1].long()
    base = torch.as_tensor(sc.region.reshape(-1).astype("float32") - 1.0, device=st.device)  # road 0, inactive -1
    obs = torch.cat([st, ns], 0).reshape(2 * K, B, -1)
    facts = {"edge": int(edge.sum()), "done": int(rp.done[tr, e].sum()),
             # a reset obs holds 0.5 (9.5 on the own apple) at the agents; every later obs holds integers
             "reset": int((st != st.round()).reshape(K, B, -1).any(-1).any(0).sum()),
             "patches": int((obs != base).sum(-1).max())}
    return got, auto, ref, facts


@pytest.mark.parametrize("sid,B", DESC, ids=[d[0] for d in DESC])
def test_desc_learner_matches_float64(sid, B):
    """Two descriptor updates with one env step between them, each against the float64 reference built
    from the weights read back before it, the recorded rows and uniforms, and the critic read back
    after its step: the same per-tensor and per-block bounds as the dense sweep, on the gradient
    buffers the update leaves and on a_next.  The second update is right only if the first one's
    launches refreshed the c1 partial sums of all four networks.  Conditions of the seed: at most B / 8
    edge rows; a done transition and a reset obs among the sampled rows of every case with B >= 48 (more
    than the "at least one case" asked for; a 16-row sample is only reported); on the 6 x 6 map an obs
    with all N + 1 patches surviving (counted on the dense obs against the map).  Only the gradients are
    compared on the clean rows: the losses and a_next are continuous in a ReLU input at zero, so they
    are compared on all rows, edge rows included."""
    sc, env, m, m3, ro = _desc_setup(sid, B)
    try:
        for upd in (1, 2):
            if upd == 2:
                ro.step()
                ro.fence()
            got, auto, ref, facts = _desc_update(sc, m, m3, ro)
            rec = {"case": sid, "B": B, "update": upd, **facts,
                   "fused": {n: float("%.2e" % e) for n, e in tensor_errors(got, ref).items()},
                   "autograd": {n: float("%.2e" % e) for n, e in tensor_errors(dict(ref, **auto), ref).items()
                                if not n.endswith(".loss")},
                   "a_next": float((got["a_next"].double() - ref["a_next"]).abs().max()),
                   "blocks": _block_record(block_report(got, auto, ref))}
            print("REF64D " + json.dumps(rec))
            assert facts["edge"] <= B // 8, facts
            if B >= 48:
                assert facts["done"] > 0 and facts["reset"] > 0, facts
            if sid.startswith("open"):
                assert facts["patches"] == sc.N + 1, facts
            f = failures(got, auto, ref)
            assert not f["probs"] and not f["tensors"] and not f["blocks"], (upd, f)
        assert m.opt_critic.count[0].item() == m.opt_actor.count[0].item() == 2
    finally:
        env.close()
