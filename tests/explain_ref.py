"""References for the explanation of a link score (TgnEngine.attention / explain).

The STRUCTURAL reference is the oracle itself: the embedding of node v with the slots S absent is oracle_embed
(tgn_oracle_steps.py) on a copy.deepcopy of the oracle loader with e_id[v, S] = -1 — the sampler's own mask
(RefLastNeighborLoader.__call__ drops e_id < 0) — and a logit is RefLinkPredictor's layers before the sigmoid.  The GPU
tests compare the device against it.

The CLOSED FORM is a numpy / float64 restatement of the leave-one-out softmax from the oracle's parameters and state
(query, keys, values, edge rows and skip row of one node; max, exponentials, + 1e-16 denominator and weighted sum over
the remaining slots).  test_explain_cpu.py asserts that it equals the structural reference.

The state of every test here: a 500-event wiki-shaped stream over 300 nodes (stream seed 3, msg_dim 16), parameters of
RefTGN under torch.manual_seed(0) as tgn_oracle_steps.Rig draws them, aggr "last"; 8 eval batches of 50 events with 5
negatives each (test_gpu_tgn_query._built's negatives: default_rng(9) over the destination nodes); the pairs explained
are the 50 events of batch 8."""
import copy
import math

import numpy as np
import torch

from tgn_oracle_steps import oracle_embed

N, B, MSG, NB, KN, SEED, BATCHES = 300, 50, 16, 10, 5, 3, 8


def stream():
    from tgnx.synth import make_stream
    return make_stream("tgbl-wiki", seed=SEED, num_events=B * NB, num_nodes=N, msg_dim=MSG)


def negatives(s):
    return torch.from_numpy(np.random.default_rng(9).choice(s.dst_nodes, size=(BATCHES * B, KN)))


def new_oracle(D, ring, layers=1):
    """(RefTGN, RefLastNeighborLoader) as tgn_oracle_steps.Rig builds them."""
    from oracle.sampler_ref import RefLastNeighborLoader
    from oracle.tgn_ref import RefTGN
    torch.manual_seed(0)
    return RefTGN(N, MSG, hidden=D, aggr="last", dropout=0.0, layers=layers), RefLastNeighborLoader(N, ring)


def advance(ref, lref, s, negs, count=BATCHES):
    """`count` eval batches on the oracle (its first eval() flushes the empty stores).  Returns (ev_t, ev_msg)."""
    from oracle.tgn_ref import eval_step
    ev_t, ev_msg = torch.from_numpy(s.t.astype(np.float32)), torch.from_numpy(s.msg)
    src, dst = torch.from_numpy(s.src), torch.from_numpy(s.dst)
    for st in range(count):
        sl = slice(st * B, (st + 1) * B)
        eval_step(ref, lref, ev_t, ev_msg, src[sl], dst[sl], negs[sl], ev_t[sl], ev_msg[sl])
    return ev_t, ev_msg


def pairs(s, st=BATCHES):
    sl = slice(st * B, (st + 1) * B)
    return s.src[sl].copy(), s.dst[sl].copy()


@torch.no_grad()
def logit(ref, za, zb):
    lp = ref.link_pred
    return lp.lin_final((lp.lin_src(za) + lp.lin_dst(zb)).relu()).view(-1)


def slot_sets(lref, v, by):
    """The valid ring positions of node v in slot order and, per valid slot j, the ring positions of S_j."""
    pos = np.flatnonzero(lref.e_id[v] >= 0)
    nb = lref.neighbors[v][pos]
    if by == "slot":
        return pos, [pos[[j]] for j in range(pos.size)]
    assert by == "neighbour", by
    return pos, [pos[nb == nb[j]] for j in range(pos.size)]


def structural_node(ref, lref, ev_t, ev_msg, v, by):
    """dict(event [ne], neighbour [ne], t [ne], z [D], loo_z [ne, D], lead [ne]) of node v from the oracle."""
    v = int(v)
    pos, sets = slot_sets(lref, v, by)
    masked = copy.deepcopy(lref)
    rows = []
    for S in sets:
        masked.e_id[v, S] = -1
        rows.append(oracle_embed(ref, masked, ev_t, ev_msg, [v])[0])
        masked.e_id[v] = lref.e_id[v]
    nb = lref.neighbors[v][pos]
    D = ref.memory.memory.size(1)
    return dict(event=lref.e_id[v][pos].copy(), neighbour=nb.copy(), t=lref.t[v][pos].copy(),
                z=oracle_embed(ref, lref, ev_t, ev_msg, [v])[0],
                loo_z=torch.stack(rows) if rows else torch.zeros(0, D),
                lead=np.array([not (nb[:j] == nb[j]).any() for j in range(pos.size)], dtype=bool))


def structural_explain(ref, lref, ev_t, ev_msg, src, dst, by):
    """The oracle's explanation of the pairs: dict(logit [P], nodes {v: structural_node}, src / dst: per pair a dict
    {event id: effect}) with effect = logit - the logit with that side's S_j absent and the other side whole."""
    nodes = {int(v): structural_node(ref, lref, ev_t, ev_msg, v, by) for v in np.unique(np.concatenate([src, dst]))}
    out = dict(logit=[], src=[], dst=[], nodes=nodes)
    for a, b in zip(src, dst):
        na, nb = nodes[int(a)], nodes[int(b)]
        base = float(logit(ref, na["z"][None], nb["z"][None]))
        out["logit"].append(base)
        ea = base - logit(ref, na["loo_z"], nb["z"][None].expand(na["loo_z"].size(0), -1)).double().numpy()
        eb = base - logit(ref, na["z"][None].expand(nb["loo_z"].size(0), -1), nb["loo_z"]).double().numpy()
        out["src"].append(dict(zip(na["event"].tolist(), ea.tolist())))
        out["dst"].append(dict(zip(nb["event"].tolist(), eb.tolist())))
    out["logit"] = np.array(out["logit"])
    return out


@torch.no_grad()
def oracle_attention(ref, lref, ev_t, ev_msg, nodes):
    """{v: {event id: alpha [2]}}: the eval-mode attention of each node's own softmax (layers = 2: conv2's, the root
    level), transformer_attention's second output over the oracle's sampled edge list."""
    from oracle.tgn_ref import sample_hops, transformer_attention
    ref.eval()
    nodes = np.unique(np.asarray(nodes, dtype=np.int64))
    n_id, ei, e_id = sample_hops(ref, lref, nodes)
    x, lu = ref.memory(n_id)
    g = ref.gnn
    enc = g.time_enc((lu[ei[0]] - ev_t[e_id]).to(x.dtype))
    attr = torch.cat([enc, ev_msg[e_id]], dim=-1)
    conv = g.conv
    if ref.layers == 2:
        x, conv = g.conv(x, ei, attr), g.conv2
    H, C = conv.H, conv.C
    j, i = ei[0], ei[1]
    q = conv.lin_query(x)[i].view(-1, H, C)
    k = conv.lin_key(x)[j].view(-1, H, C)
    val = conv.lin_value(x)[j].view(-1, H, C)
    e = conv.lin_edge(attr).view(-1, H, C)
    _, alpha = transformer_attention(q, k, val, e, i, x.size(0))
    centre = n_id[i].numpy()
    out = {int(v): {} for v in nodes}
    for row in range(e_id.numel()):
        c = int(centre[row])
        if c in out:
            out[c][int(e_id[row])] = alpha[row].double().numpy()
    return out


@torch.no_grad()
def closed_form_node(ref, lref, ev_t, ev_msg, v, by):
    """float64 numpy: dict(z [D], alpha [ne, 2], loo_z [ne, D]) of node v at layers = 1, from the parameters."""
    assert ref.layers == 1
    v = int(v)
    pos, sets = slot_sets(lref, v, by)
    conv, mem = ref.gnn.conv, ref.memory
    H, C = conv.H, conv.C
    f = lambda t: t.detach().double().numpy()  # noqa: E731

    def lin(layer, x):
        y = x @ f(layer.weight).T
        return y if layer.bias is None else y + f(layer.bias)

    xv = f(mem.memory[v])
    skip, q = lin(conv.lin_skip, xv), lin(conv.lin_query, xv).reshape(H, C)
    D = xv.shape[0]
    if pos.size == 0:
        return dict(z=skip, alpha=np.zeros((0, H)), loo_z=np.zeros((0, D)))
    nb, ev = lref.neighbors[v][pos], lref.e_id[v][pos]
    rel = (mem.last_update[nb] - ev_t[ev]).float()
    te = ref.gnn.time_enc.lin
    arg = (rel.double().view(-1, 1) * te.weight.double().view(1, -1) + te.bias.double()).float()   # RefTimeEncoder
    e = lin(conv.lin_edge, np.concatenate([np.cos(f(arg)), f(ev_msg[ev])], axis=1)).reshape(-1, H, C)
    xu = f(mem.memory[nb])
    key, val = lin(conv.lin_key, xu).reshape(-1, H, C) + e, lin(conv.lin_value, xu).reshape(-1, H, C) + e
    a = (q[None] * key).sum(-1) / math.sqrt(C)                                                      # [ne, H]

    def attend(keep):
        if not keep.any():
            return np.zeros((pos.size, H)), skip
        ex = np.where(keep[:, None], np.exp(a - a[keep].max(0)), 0.0)
        al = ex / (ex.sum(0) + 1e-16)
        return al, (al[:, :, None] * val).sum(0).reshape(-1) + skip

    alpha, z = attend(np.ones(pos.size, dtype=bool))
    loo = [attend(~np.isin(pos, S))[1] for S in sets]
    return dict(z=z, alpha=alpha, loo_z=np.stack(loo))
