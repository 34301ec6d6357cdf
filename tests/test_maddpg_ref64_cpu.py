"""The float64 restatement of the update (tests/_maddpg_ref64.py) against the reference the project
already trusts, tests/test_maddpg.py's PerAgentReference (one nn.Sequential and one optimizer per
agent and network), with that loop's modules converted to float64 on the CPU: losses, target
actions and every gradient within 1e-12 relative L2 (both are float64 and differ only in summation
order: stacked matmuls against per-agent nn.Linear / nn.LayerNorm).

PerAgentReference runs in float64 as it stands.  Two things are arranged around it: its loop forms
the rewards and (1 - done) * gamma in float32, so the rewards used here are float32 numbers and
gamma is 31/32; and its optimizers are replaced by recorders that keep each gradient when ``step``
is called and step nothing, so the actor phase sees the initial critic (the learning rate 0 of the
GPU sweep) and the critic's gradient is read before the actor loss's backward adds to it.

Also here: every dense case of the GPU sweep keeps its masked rows within B / 8 and its forced rows
unmasked (float64, CPU, the case's seed), so the GPU sweep is never where that is found out."""
import pytest
import torch

import _learner_cases as C
import _maddpg_ref64 as R
from test_maddpg import PerAgentReference

TOL = 1e-12


class _Recorder:
    """Stands in for one agent's optimizer: keeps the gradients at ``step`` and changes nothing."""

    def __init__(self, module):
        self.module, self.grads = module, None

    def zero_grad(self):
        for p in self.module.parameters():
            p.grad = None

    def step(self):
        self.grads = [p.grad.detach().clone() for p in self.module.parameters()]


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _stack(recs):
    """K agents' nn.Sequential gradients (Linear, LayerNorm, ReLU, Linear, LayerNorm, ReLU, Linear:
    weight [out, in], bias, ...) in GRAD_NAMES order and StackedMLPActors' shapes."""
    out = []
    for j in range(10):
        ts = [r.grads[j] for r in recs]
        out.append(torch.stack([t.t() if t.dim() == 2 else t.unsqueeze(0) for t in ts]))
    return out


@pytest.mark.parametrize("K", [1, 3])
def test_ref64_equals_per_agent_loop_in_float64(K):
    H, W, B, seed = 4, 5, 24, 11
    m = C.make_learner(K, H, W, B, seed, "cpu")
    C.perturb(m, seed)
    m.gamma = 0.96875  # an f32 number: the loop's (1 - done).float() * gamma is an f32 product
    b, _ = C.batch(K, H, W, B, seed)
    st, ac, rw, ns, dn, un, uc = b
    rw = rw.float().double()  # the loop rounds rewards to f32 (the forced 1e6 + 1/3 included)
    ref = PerAgentReference(m, 0.0, 0.0)
    for seqs in (ref.actors, ref.actor_t, ref.critics, ref.critic_t):
        for s in seqs:
            s.double()  # f32 values are f64 values: the same networks as params64(m)
    ref.opt_c = [_Recorder(c) for c in ref.critics]
    ref.opt_a = [_Recorder(a) for a in ref.actors]
    with torch.no_grad():
        a_next = torch.stack([R.gumbel_softmax(ref.actor_t[k](ns[k].reshape(B, -1).double()), un[k].double())
                              for k in range(K)])
    losses = ref.learn(st.double(), ac.double(), rw, ns.double(), dn, un.double(), uc.double())
    c, a = R.update(R.params64(m), st, ac, rw, ns, dn, un, uc, m.gamma)
    assert _rel(c["a_next"], a_next) < TOL
    for k in range(K):
        assert abs(float(a["loss"][k]) - losses[k][0]) <= TOL * abs(losses[k][0])
        assert abs(float(c["loss"][k]) - losses[k][1]) <= TOL * abs(losses[k][1])
    worst = 0.0
    for got, want in ((c["grads"], _stack(ref.opt_c)), (a["grads"], _stack(ref.opt_a))):
        for name, g, w in zip(R.GRAD_NAMES, got, want):
            assert g.shape == w.shape, name
            worst = max(worst, _rel(g, w))
            assert _rel(g, w) < TOL, (name, _rel(g, w))
    print("worst gradient rel L2 vs the per-agent loop (f64):", worst)


def test_row_weights_remove_exactly_one_rows_terms():
    """Zeroing a row's weight equals the update of the batch without that row, scaled by (B - 1) / B."""
    K, H, W, B, seed = 2, 3, 3, 16, 5
    m = C.make_learner(K, H, W, B, seed, "cpu")
    C.perturb(m, seed)
    P = R.params64(m)
    b, _ = C.batch(K, H, W, B, seed)
    w = torch.ones(B, dtype=torch.float64)
    w[5] = 0
    keep = [r for r in range(B) if r != 5]
    sub = [t[:, keep] if t.shape[0] == K and t.dim() > 2 else t[keep] for t in b]
    c0, a0 = C.reference(P, b, row_w=w)
    c1, a1 = C.reference(P, sub)
    for x0, x1 in ((c0, c1), (a0, a1)):
        for g0, g1 in zip(x0["grads"] + [x0["loss"]], x1["grads"] + [x1["loss"]]):
            assert _rel(g0, g1 * (B - 1) / B) < TOL


@pytest.mark.parametrize("i", range(len(C.DENSE)), ids=C.DENSE_IDS)
def test_dense_case_masks_few_rows(i):
    c = C.dense_case(i)
    print(C.DENSE_IDS[i], "masked rows:", c["masked"])
    assert c["edge_left"] == 0
    assert len(c["masked"]) <= c["B"] // 8, c["masked"]
    assert not set(c["masked"]) & set(c["forced"]), (c["masked"], c["forced"])
    st, ac, rw, ns, dn, un, uc = c["batch"]
    K = c["K"]
    assert dn[0].all() and not dn[1].any() and rw[2, K - 1] == 1e6 + 1.0 / 3.0
    assert un[0, 3, 0] == 0.0 and uc[0, 3, 0] == 0.0 and un[K - 1, 4, 8] == uc[K - 1, 4, 8] < 1.0
    assert float(un[K - 1, 4, 8]) == 1.0 - 2.0 ** -24
