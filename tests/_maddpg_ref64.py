"""One MADDPG update (marlnav/maddpg.py's docstring; agilerl 1.0.15 MADDPG.learn) restated in plain
float64 torch: no project kernel, no project autograd function.  It is the yardstick of
tests/test_gpu_learner_shapes.py (the fused and the descriptor learner against it) and is itself
tied to tests/test_maddpg.py's PerAgentReference in tests/test_maddpg_ref64_cpu.py.

Runs where its inputs live (CPU, or the device for device tensors).  A network is a dict
``{"w": [3], "b": [3], "lw": [2], "lb": [2]}`` of float64 tensors in StackedMLPActors' shapes
(w [K, in, out], b / lw / lb [K, 1, out]); the layer form is Linear -> LayerNorm (biased variance,
eps 1e-5) -> affine -> ReLU, twice, then Linear.  Gradients come from float64 autograd over this
composition and are returned in the order of GRAD_NAMES (tests/test_maddpg_fused.py::_grads).

``row_w`` [B] (default ones) weighs each row's loss term; the mean still divides by B, so zeroing
a row's weight removes exactly that row's contribution from every gradient and loss.
"""
import torch

GRAD_NAMES = ("w1", "b1", "ln1_w", "ln1_b", "w2", "b2", "ln2_w", "ln2_b", "w3", "b3")
LN_EPS, G_EPS = 1e-5, 1e-20
F64 = torch.float64


def net64(net, device=None) -> dict:
    """A StackedMLPActors' parameters, upcast (detached copies)."""
    def up(t):
        return t.detach().to(device=device if device is not None else t.device, dtype=F64).clone()
    return {"w": [up(t) for t in net.weights], "b": [up(t) for t in net.biases], "lw": [up(t) for t in net.ln_w],
            "lb": [up(t) for t in net.ln_b]}


def params64(m, device=None) -> dict:
    """The four networks of a MADDPG."""
    return {"actor": net64(m.actors.net, device), "actor_target": net64(m.actor_targets.net, device),
            "critic": net64(m.critics, device), "critic_target": net64(m.critic_targets, device)}


def leaves(p: dict) -> list:
    """A network's tensors in GRAD_NAMES order."""
    return [p["w"][0], p["b"][0], p["lw"][0], p["lb"][0], p["w"][1], p["b"][1], p["lw"][1], p["lb"][1], p["w"][2],
            p["b"][2]]


def _with_grad(p: dict) -> dict:
    return {k: [t.detach().clone().requires_grad_(True) for t in v] for k, v in p.items()}


def mlp(p: dict, x: torch.Tensor, taps: list) -> torch.Tensor:
    """x [K, B, in] -> [K, B, out]; appends the two ReLU inputs [K, B, h] (detached) to ``taps``."""
    h = x
    for i in range(3):
        z = torch.matmul(h, p["w"][i]) + p["b"][i]
        if i == 2:
            return z
        mu = z.mean(-1, keepdim=True)
        var = ((z - mu) ** 2).mean(-1, keepdim=True)
        a = (z - mu) / torch.sqrt(var + LN_EPS) * p["lw"][i] + p["lb"][i]
        taps.append(a.detach())
        h = torch.relu(a)


def gumbel_softmax(logits, u):
    """agilerl's GumbelSoftmax, tau 1: softmax(logits - log(-log(u + eps) + eps))."""
    return torch.softmax(logits - torch.log(-torch.log(u + G_EPS) + G_EPS), -1)


def critic_in(obs, actions):
    """obs [K, B, D], actions [K, B, 9] -> [B, K*D + 9K], agent-major."""
    B = obs.shape[1]
    return torch.cat([obs.permute(1, 0, 2).reshape(B, -1), actions.permute(1, 0, 2).reshape(B, -1)], 1)


def _obs(states):
    return states.to(F64).reshape(states.shape[0], states.shape[1], -1)


def critic_phase(P: dict, states, actions, rewards, next_states, dones, u_next, gamma: float, row_w=None) -> dict:
    """Phase 1: a'_k = GumbelSoftmax(actor_target_k(s'_k)); y = r + (1 - d) gamma critic_target_k(x');
    loss_k = mean_b (critic_k(x) - y)^2 and its gradient for every critic parameter.
    -> a_next [K, B, 9], y [K, B, 1], loss [K], grads (GRAD_NAMES order), relu_in: the ReLU inputs
    of (actor_target, critic_target, critic), two [K, B, 128] tensors each."""
    K, B = states.shape[0], states.shape[1]
    s, ns, act = _obs(states), _obs(next_states), actions.to(F64)
    taps = {"actor_target": [], "critic_target": [], "critic": []}
    with torch.no_grad():
        a_next = gumbel_softmax(mlp(P["actor_target"], ns, taps["actor_target"]), u_next.to(F64))
        x_next = critic_in(ns, a_next)
        q_next = mlp(P["critic_target"], x_next.unsqueeze(0).expand(K, -1, -1), taps["critic_target"])
        r = rewards.to(F64).t().unsqueeze(-1)
        d = dones.to(F64).t().unsqueeze(-1)
        y = r + (1.0 - d) * gamma * q_next
    c = _with_grad(P["critic"])
    q = mlp(c, critic_in(s, act).unsqueeze(0).expand(K, -1, -1), taps["critic"])
    w = torch.ones(B, dtype=F64, device=s.device) if row_w is None else row_w.to(F64)
    loss = (w[None, :, None] * (q - y) ** 2).sum(dim=(1, 2)) / B
    grads = torch.autograd.grad(loss.sum(), leaves(c))
    return {"a_next": a_next, "y": y, "loss": loss.detach(), "grads": [g.detach() for g in grads], "relu_in": taps}


def actor_phase(actor: dict, critic: dict, states, actions, u_cur, row_w=None) -> dict:
    """Phase 2 through the given critic (a constant): probs_k = GumbelSoftmax(actor_k(s_k)),
    loss_k = -mean_b critic_k(s, a with a_k := probs_k) and its gradient for every actor parameter.
    -> probs [K, B, 9], loss [K], q_abs [K] = mean_b |Q| (the scale of the loss's terms: the loss itself
    can cancel), grads, relu_in of (actor, critic on the mixed actions)."""
    K, B = states.shape[0], states.shape[1]
    s, act = _obs(states), actions.to(F64)
    taps = {"actor": [], "critic_mix": []}
    a = _with_grad(actor)
    probs = gumbel_softmax(mlp(a, s, taps["actor"]), u_cur.to(F64))
    rows = []
    for k in range(K):
        mixed = [act[j] for j in range(K)]
        mixed[k] = probs[k]
        rows.append(critic_in(s, torch.stack(mixed)))
    q = mlp(critic, torch.stack(rows), taps["critic_mix"])
    w = torch.ones(B, dtype=F64, device=s.device) if row_w is None else row_w.to(F64)
    loss = -(w[None, :, None] * q).sum(dim=(1, 2)) / B
    grads = torch.autograd.grad(loss.sum(), leaves(a))
    return {"probs": probs.detach(), "loss": loss.detach(), "q_abs": q.detach().abs().mean(dim=(1, 2)),
            "grads": [g.detach() for g in grads], "relu_in": taps}


def update(P: dict, states, actions, rewards, next_states, dones, u_next, u_cur, gamma: float, critic_after=None,
           row_w=None):
    """Both phases; the actor phase sees ``critic_after`` (e.g. read back from the device after the
    critic's Adam step) or, by default, the initial critic (a critic learning rate of 0)."""
    c = critic_phase(P, states, actions, rewards, next_states, dones, u_next, gamma, row_w)
    a = actor_phase(P["actor"], critic_after if critic_after is not None else P["critic"], states, actions, u_cur,
                    row_w)
    return c, a


def edge_rows(phases, edge: float) -> torch.Tensor:
    """Rows [B] (bool) with a ReLU input of any evaluated network within ``edge`` of zero."""
    rows = None
    for ph in phases:
        for taps in ph["relu_in"].values():
            for a in taps:
                hit = (a.abs() < edge).any(-1).any(0)
                rows = hit if rows is None else rows | hit
    return rows
