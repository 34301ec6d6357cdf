"""The dense cases of the learner shape sweep (tests/test_gpu_learner_shapes.py), built on the CPU
so that everything the GPU test assumes about them is checked without a GPU
(tests/test_maddpg_ref64_cpu.py): the learner's weights, the batch with its forced rows, the
float64 reference of the update and the rows masked for a ReLU input at the rounding edge.

tests/test_maddpg_fused.py's ``_batch`` / ``_pair`` draw on the device with a device generator, so
their numbers cannot be reproduced on the CPU; ``batch`` / ``perturb`` here draw the same
distributions with a CPU generator and the GPU test moves the tensors over.  A MADDPG's initial
weights already come from a CPU generator on either device."""
import functools

import torch

import _maddpg_ref64 as R

EDGE = 1e-5  # tests/test_maddpg_fused.py's: a ReLU input this close to 0 could flip between two f32 orders
GAMMA, LR = 0.98, 1e-3

# (K, H, W, B, seed, what the row reaches).  seed: chosen so that the masked rows stay within B / 8 and
# none of the forced rows is masked (both asserted on the CPU).
DENSE = [
    (1, 1, 1, 16, 3, "one input; one k-step; nw1 = 1; ldx = 10"),
    (2, 1, 3, 48, 3, "D % 4 != 0; all of layer 1 in a partial chunk"),
    (3, 7, 9, 144, 3, "one short of a chunk; K*D = 189; second row tile of 16 rows"),
    (1, 8, 8, 128, 3, "exact chunk; ldx = 73: a last chunk of 9 action inputs"),
    (2, 5, 13, 16, 3, "last chunk of exactly one input"),
    (8, 6, 6, 32, 3, "K = MAXK; s_act at full width 72"),
    (3, 19, 19, 272, 3, "K*D = 1083: 17 chunks (RED_PRE + 1); ldx = 1110: 18; three row tiles, last of 16"),
    (5, 5, 8, 256, 3, "odd K; two full row tiles"),
]


def case_id(c) -> str:
    return f"k{c[0]}_{c[1]}x{c[2]}_b{c[3]}"


DENSE_IDS = [case_id(c) for c in DENSE]


def make_learner(K, H, W, B, seed, device, lr_critic=0.0, **kw):
    from marlnav.maddpg import MADDPG
    return MADDPG(K, H, W, lr_actor=LR, lr_critic=lr_critic, gamma=GAMMA, tau=0.01, batch_size=B, device=device,
                  seed=seed, **kw)


def perturb(m, seed):
    """Targets apart from the online networks and non-trivial LayerNorm affines on all four (drawn
    on the CPU, the same numbers on any device)."""
    g = torch.Generator().manual_seed(seed + 50)
    with torch.no_grad():
        for net in (m.actor_targets.net, m.critic_targets):
            flat = net.flat_params()
            flat.add_((0.05 * torch.randn(flat.shape, generator=g)).to(flat.device))
        for net in (m.actors.net, m.critics, m.actor_targets.net, m.critic_targets):
            for lw, lb in zip(net.ln_w, net.ln_b):
                lw.add_((0.2 * torch.randn(lw.shape, generator=g)).to(lw.device))
                lb.add_((0.1 * torch.randn(lb.shape, generator=g)).to(lb.device))


def batch(K, H, W, B, seed):
    """_batch's distributions on the CPU, then the forced rows: row 0 all dones 1, row 1 all 0, a reward
    of 1e6 + 1/3 (not an f32 number) for the last agent in row 2, a uniform of exactly 0 in row 3 and
    the largest float below 1 in row 4 (both Gumbel samples).  -> (tensors, forced row indices)"""
    g = torch.Generator().manual_seed(seed + 7)
    states = torch.randint(-1, 6, (K, B, H, W), generator=g).float()
    next_states = torch.randint(-1, 6, (K, B, H, W), generator=g).float()
    actions = torch.softmax(torch.randn((K, B, 9), generator=g) * 2, -1)
    rewards = torch.randn((B, K), generator=g, dtype=torch.float64) * 10
    dones = (torch.rand((B, K), generator=g) < 0.2).to(torch.uint8)
    u_next = torch.rand((K, B, 9), generator=g)
    u_cur = torch.rand((K, B, 9), generator=g)
    below1 = float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))
    dones[0], dones[1] = 1, 0
    rewards[2, K - 1] = 1e6 + 1.0 / 3.0
    for u in (u_next, u_cur):
        u[0, 3, 0] = 0.0
        u[K - 1, 4, 8] = below1
    return [states, actions, rewards, next_states, dones, u_next, u_cur], (0, 1, 2, 3, 4)


def reference(P, b, critic_after=None, row_w=None):
    st, ac, rw, ns, dn, un, uc = b
    return R.update(P, st, ac, rw, ns, dn, un, uc, GAMMA, critic_after=critic_after, row_w=row_w)


@functools.lru_cache(maxsize=None)
def dense_case(i: int) -> dict:
    """Case i on the CPU: the perturbed learner's float64 parameters, the batch after masking (edge rows
    replaced by a copy of a clean row, as test_fused_gradients_match_autograd does), the masked rows
    and the float64 reference of the update on it.  Computed once per session; never modified."""
    K, H, W, B, seed, _ = DENSE[i]
    m = make_learner(K, H, W, B, seed, "cpu")
    perturb(m, seed)
    P = R.params64(m)
    b, forced = batch(K, H, W, B, seed)
    masked = []
    for _ in range(4):
        rows = R.edge_rows(reference(P, b), EDGE)
        if not rows.any():
            break
        clean = next(r for r in range(B) if not rows[r] and r not in forced)  # not a forced row: no tilt to done = 1
        st, ac, rw, ns, dn, un, uc = b
        for r in rows.nonzero().flatten().tolist():
            masked.append(r)
            for t in (st, ac, ns, un, uc):
                t[:, r] = t[:, clean]
            rw[r], dn[r] = rw[clean], dn[clean]
    c, a = reference(P, b)  # of the batch as returned, however the loop ended
    rows = R.edge_rows((c, a), EDGE)
    return dict(K=K, H=H, W=W, B=B, seed=seed, P=P, batch=b, forced=forced, masked=masked, edge_left=int(rows.sum()),
                critic=c, actor=a)
