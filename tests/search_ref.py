"""Host restatement of the batched search (include/tensor_game_search.h) for ONE game, in numpy float32: the semantics
of the reference's actor_prediction / mc_ts / extend_tree / backward_pass / get_improved_policy (act.py:8-301) on the
64-bit head keys of the build, with the build's two deviations (a terminal leaf inside the horizon is worth 0; a
descent is cut at max_depth) and int8 wrap of child heads.  The improved policy is formed with torch exactly as the
reference forms it (float32 log / pow on the host).

``policy_fn(head int8 (S,S,S), frames int8 (T,S,S,S), scalar int, attempt int, key int) -> (tokens (k,3S), q float32)``.
``play`` also logs every policy call and whether a candidate child head left int8 (the header's ``overflow``).
"""
import numpy as np
import torch

from oracle import tensor_game as O

F32 = np.float32


def head_key(head) -> int:
    return int(O.state_hash(np.asarray(head, np.int8)[None])[0])


def child_frames(frames, tokens, shift=1):
    """[frames[0] - tensor(tokens), frames[0..T-2]] with int8 wrap (get_child_states, act.py:266-275)."""
    frames = np.asarray(frames, np.int8)
    head = (frames[0].astype(np.int64) - O.action_to_tensor(np.asarray(tokens), shift)).astype(np.int8)
    return np.concatenate([head[None], frames[:-1]], axis=0)


def argmax_first(v) -> int:
    """torch.argmax: first maximal index, NaN counts as the maximum."""
    v = np.asarray(v, F32)
    nan = np.isnan(v)
    if nan.any():
        return int(np.argmax(nan))
    return int(np.argmax(v))


class Node:
    def __init__(self, frames, tokens, keys):
        self.frames = np.array(frames, np.int8)
        self.tokens = np.array(tokens, np.int8)
        self.keys = [int(x) for x in keys]
        self.N = np.zeros(len(self.keys), F32)
        self.Q = np.zeros(len(self.keys), F32)


def improved_policy(N, tokens, n_bar, n_logits):
    """get_improved_policy (act.py:278-301) for one root, with torch as the reference computes it."""
    vc = torch.from_numpy(np.asarray(N, F32)[None].copy())
    s = vc.sum()
    nb = torch.tensor(n_bar)
    tau = (s.log() / nb.log()).item() if s > nb else 1
    ip = (vc ** (1 / tau)) / s
    out = torch.zeros(tokens.shape[1], n_logits)
    for j in range(tokens.shape[0]):
        for step, tok in enumerate(tokens[j]):
            out[step, int(tok)] += ip[0, j]
    return out.numpy()


def play(policy_fn, start, max_actions, n_sim, n_bar, n_logits, horizon=5, max_depth=64, shift=1, max_retries=256):
    """One game.  Returns a dict: states (L,T,S,S,S) int8, policy (L,3S,n_logits) f32, rewards (L,) int64, length,
    root_N / root_Q (lists of f32 arrays), choice (L,) and status (bit 1: a descent over max_depth); further
    ``calls``, one ``(frames int8 (T,S,S,S), scalar, attempt, key)`` per policy call in order, ``overflow`` (a candidate
    child head of some expansion attempt left int8 before the wrap -- over all k candidates, kept or dropped) and
    ``n_nodes``, the size of the tree at the end."""
    frames = np.array(start, np.int8)
    nodes = {}
    root, root_key = frames, head_key(frames[0])
    states, roots, choice = [], [], []
    status = 0
    move = 0
    calls, overflow = [], False
    while move < max_actions:
        states.append(root)
        sims = n_sim
        if root_key in nodes:
            sims = max(n_sim - int(nodes[root_key].N.sum()), 0)
        for _ in range(sims):
            key, fr, depth, path = root_key, root, 0, []
            cut = False
            while key in nodes:
                if depth >= max_depth:
                    cut = True
                    break
                nd = nodes[key]
                j = argmax_first(nd.Q)
                path.append((key, j))
                fr, key = child_frames(nd.frames, nd.tokens[j], shift), nd.keys[j]
                depth += 1
            if cut:
                status |= 2
                continue
            reward = 0
            if move + depth <= min(max_actions, move + horizon):
                head = fr[0]
                if head.any():
                    for attempt in range(max_retries + 1):
                        tokens, q = policy_fn(head, fr, move + depth, attempt, key)
                        tokens = np.asarray(tokens)
                        calls.append((fr.copy(), move + depth, attempt, key))
                        exact = head[None].astype(np.int64) - O.action_to_tensor(tokens, shift)
                        overflow |= bool(((exact < -128) | (exact > 127)).any())
                        kids = exact.astype(np.int8)
                        changed = (kids != head[None]).reshape(len(tokens), -1).any(axis=1)
                        kid_keys = O.state_hash(kids)
                        keep = [i for i in range(len(tokens)) if changed[i] and int(kid_keys[i]) not in nodes]
                        if keep:
                            break
                    else:
                        raise RuntimeError("no surviving candidate")
                    nodes[key] = Node(fr, tokens[keep], kid_keys[keep])
                    reward = F32(F32(0) + F32(q))
            reward = F32(reward)
            for nk, j in reversed(path):
                reward = F32(reward - F32(1))
                nd = nodes[nk]
                n, q = nd.N[j], nd.Q[j]
                nd.Q[j] = F32(F32(F32(n * q) + reward) / F32(n + F32(1)))
                nd.N[j] = F32(n + F32(1))
        nd = nodes[root_key]
        j = argmax_first(nd.Q)
        roots.append(root_key)
        choice.append(j)
        root, root_key = child_frames(nd.frames, nd.tokens[j], shift), nd.keys[j]
        move += 1
        if not root[0].any():
            break
    L = len(states)
    pol = np.stack([improved_policy(nodes[k].N, nodes[k].tokens, n_bar, n_logits) for k in roots])
    rank = int(O.slice_rank_exact(root[0][None])[0])
    rewards = np.cumsum(np.array([-1] * (L - 1) + [-1 - rank], np.int64))
    return dict(states=np.stack(states), policy=pol, rewards=rewards, length=L, choice=np.array(choice, np.int32),
                root_N=[nodes[k].N.copy() for k in roots], root_Q=[nodes[k].Q.copy() for k in roots], status=status,
                final=root, calls=calls, overflow=overflow, n_nodes=len(nodes))


# ---- the device stand-in of mat_mul_amd.search.keyed_policy, on the host -----------------------------------------
_C1, _C2, _C3, _C4 = (np.uint64(c) for c in (0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB,
                                              0xD6E8FEB86659FD93))


def _mix(x):
    x = np.asarray(x, np.uint64)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * _C2
        x = (x ^ (x >> np.uint64(27))) * _C3
        return x ^ (x >> np.uint64(31))


def keyed_policy(pool, k, seed=0, p_pool=0.75):
    """policy_fn for ``play`` equal to ``mat_mul_amd.search.keyed_policy``."""
    pool = np.asarray(pool, np.int8)
    P, L = pool.shape
    thr = np.uint64(int(p_pool * (1 << 24)))
    j = np.arange(k, dtype=np.uint64)
    t = np.arange(L, dtype=np.uint64)

    def fn(head, frames, scalar, attempt, key):
        with np.errstate(over="ignore"):
            h = _mix(np.uint64(key) ^ _mix(np.uint64(attempt) * _C1 + np.uint64(seed)))
            hj = _mix(h + (j + np.uint64(1)) * _C4)
            from_pool = ((hj >> np.uint64(40)) < thr) & (attempt == 0)
            pick = ((_mix(hj + _C1) >> np.uint64(33)) % np.uint64(P)).astype(np.int64)
            rand = ((_mix(hj[:, None] + (t[None, :] + np.uint64(1)) * _C2) >> np.uint64(40)) % np.uint64(3)).astype(np.int8)
            tokens = np.where(from_pool[:, None], pool[pick], rand)
            q = F32(F32(int(_mix(h + _C3) >> np.uint64(40))) * F32(2.0 ** -23) - F32(1.0))
        return tokens, q

    return fn
