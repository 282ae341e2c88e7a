"""Host restatement of node-space growth for the grow tests (torch on the CPU only; no device, no library): what a
stream_state() dict taken at N0 nodes must look like after grow_nodes(N1), written from the rules, not from the kernel.

  rows [0, N0) of every [N, .] tensor are unchanged, bit for bit;
  rows [N0, N1) are what reset_state leaves on a fresh engine:
      memory 0, last_update 0, node_gen 0, store_nodes {0, 0, 0, 0} (empty runs),
      neighbors -1 (the constructor's fill: reset_state never rewrites it), e_id -1, ring_t -1.0;
  the event rows, the arena entries (run offsets are arena-relative) and every ctl word are unchanged;
  num_nodes becomes N1; format, ring, mem_dim, msg_dim, num_events stay."""
import torch

RESET_ROW = {"memory": 0, "last_update": 0, "node_gen": 0, "store_nodes": 0, "neighbors": -1, "e_id": -1, "ring_t": -1.0}
UNTOUCHED = ("src", "dst", "t", "msg", "store_arena", "ctl")


def pad_state(state: dict, n1: int) -> dict:
    """The stream_state() dict of the same stream on an engine grown to n1 >= state['num_nodes'] nodes."""
    n0 = int(state["num_nodes"])
    if n1 < n0:
        raise ValueError(f"pad_state: {n1} < {n0} (nodes are never dropped)")
    out = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in state.items()}
    out["num_nodes"] = int(n1)
    for k, fill in RESET_ROW.items():
        x = state[k]
        pad = torch.full((n1 - n0,) + tuple(x.shape[1:]), fill, dtype=x.dtype, device=x.device)
        out[k] = torch.cat([x, pad], 0)
    return out


def crop_state(state: dict, n0: int) -> dict:
    """The first n0 node rows of a state (what a twin built at more nodes must hold where the smaller engine has
    rows), and the rows beyond, which must be reset rows: (cropped dict, {key: rows [n0, N)})."""
    out = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in state.items()}
    out["num_nodes"] = int(n0)
    rest = {}
    for k in RESET_ROW:
        out[k], rest[k] = state[k][:n0].clone(), state[k][n0:].clone()
    return out, rest


def is_reset_rows(rest: dict) -> bool:
    return all(bool((x == RESET_ROW[k]).all()) for k, x in rest.items())


def bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def same_state(a: dict, b: dict, skip_ctl=()) -> list:
    """Keys on which two stream_state() dicts differ (bitwise for tensors); ctl words in skip_ctl are left out."""
    diff = []
    for k in a:
        x, y = a[k], b.get(k)
        if torch.is_tensor(x):
            if k == "ctl" and skip_ctl:
                keep = [i for i in range(x.numel()) if i not in skip_ctl]
                x, y = x[keep], y[keep]
            if y is None or x.shape != y.shape or not torch.equal(bits(x.cpu()), bits(y.cpu())):
                diff.append(k)
        elif x != y:
            diff.append(k)
    return diff
