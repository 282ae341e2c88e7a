"""Drop-in `LastNeighborLoader` on the HIP ring kernels.

Same constructor, attributes (`neighbors`, `e_id`, `t`, `_assoc`, `size`,
`cur_e_id`) and methods (`__call__`, `insert`, `reset_state`) as
/root/reference/neighbor_loader.py:15-109; the work runs in libtgnx
(`tgnx_ring_sample` / `tgnx_ring_insert` / `tgnx_ring_reset`).
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib


class LastNeighborLoader:
    def __init__(self, num_nodes: int, size: int, device=None):
        self.device = _lib.require_device(device)
        self.size = int(size)
        self.num_nodes = int(num_nodes)
        dev = self.device
        self.neighbors = torch.full((num_nodes, size), -1, dtype=torch.long, device=dev)
        self.e_id = torch.empty((num_nodes, size), dtype=torch.long, device=dev)
        self.t = torch.empty((num_nodes, size), dtype=torch.float, device=dev)
        self._assoc = torch.zeros(num_nodes, dtype=torch.long, device=dev)
        self._ws = torch.empty(0, dtype=torch.uint8, device=dev)
        self._ws_q = -1
        self._counts = torch.zeros(2, dtype=torch.long, device=dev)
        # bumped by every host-side change of the ring (reset_state / insert): an engine that prepared the
        # next batch from the ring (pipelined TGN step) re-prepares it when the version moved
        self.version = 0
        self.reset_state()

    # neighbor_loader.py:106-109
    def reset_state(self):
        self.cur_e_id = 0
        self.version += 1
        _lib.call("tgnx_ring_reset", _lib.ptr(self.e_id), _lib.ptr(self.t), self.num_nodes, self.size,
                  _lib.stream(self.device))

    @property
    def node_capacity(self) -> int:
        """Rows of the ring's allocations (neighbors / e_id / t / _assoc are their first num_nodes rows once grown)."""
        alloc = getattr(self, "_alloc", None)
        return self.num_nodes if alloc is None else int(alloc[0].shape[0])

    def _install(self, nbr, e_id, t, assoc, num_nodes: int) -> None:
        """Take allocations of >= num_nodes rows whose first rows hold the ring: the attributes become their first
        num_nodes rows (contiguous views), version is bumped (an engine's prefetched batch is stale) and the sample
        workspace, whose bitmap is sized by num_nodes, is dropped."""
        n = int(num_nodes)
        self._alloc = (nbr, e_id, t, assoc)
        self.neighbors, self.e_id, self.t, self._assoc = nbr[:n], e_id[:n], t[:n], assoc[:n]
        self.num_nodes = n
        self.version += 1
        self._ws = torch.empty(0, dtype=torch.uint8, device=self.device)
        self._ws_q = -1

    def grow(self, num_nodes: int, capacity=None) -> int:
        """Extend the ring to num_nodes rows in place of a rebuild: rows [0, N) are unchanged, the new rows are what
        reset_state leaves (neighbors -1, e_id -1, t -1.0, _assoc 0).  num_nodes <= N is a no-op.  Rows come out of
        the allocations' spare capacity when there is some, else everything moves into allocations of
        max(num_nodes, capacity) rows (tgnx_tgn_grow_nodes).  Bumps version and drops the sample workspace.  A loader
        bound to a TgnEngine is grown by the engine (TgnEngine.grow_nodes), which moves the model's tensors with it:
        call this only on a loader used alone (__call__ / insert).  Returns num_nodes afterwards."""
        from . import tgn
        n, N = int(num_nodes), self.num_nodes
        if n <= N:
            return N
        if n >= 1 << 31:
            raise ValueError(f"LastNeighborLoader.grow: {n} nodes; node ids are below 2^31")
        alloc = getattr(self, "_alloc", None) or (self.neighbors, self.e_id, self.t, self._assoc)
        if n > alloc[0].shape[0]:
            torch.cuda.synchronize(self.device)
            old = dict(nbr=self.neighbors, eid=self.e_id, rt=self.t, assoc=self._assoc)
            new = tgn.grow_node_tensors(self.device, N, n, max(n, int(capacity or 0)), self.size, 1, 1, old)
            alloc = (new["nbr"], new["eid"], new["rt"], new["assoc"])
        self._install(*alloc, n)
        return n

    @torch.no_grad()
    def forget(self, ids) -> dict:
        """Erase the nodes `ids` (duplicates allowed) from the ring of a loader used alone (tgnx_ring_forget): their
        own rows become what reset_state leaves (neighbors -1, e_id -1, t -1.0) and every valid slot (e_id >= 0 and
        neighbors != -1) of another row that names one of them is removed — the row's surviving entries keep their
        order at the front, the freed slots become -1 / -1 / -1.0.  A loader alone has no event table, so the t
        column drops the slots e_id drops (TgnEngine.forget_nodes re-ranks it from the table; the two agree on a
        time-ordered stream).  Returns {"nodes", "ring_slots", "ring_rows"}; bumps version.  An id outside [0, N):
        ValueError; a valid slot naming a node outside [0, N): RuntimeError; both with the ring untouched.  An empty
        list is a no-op.  A loader bound to a TgnEngine is handled by the engine (forget_nodes), which clears the
        model's rows and the message stores with it."""
        from . import tgn
        ids = torch.as_tensor(ids).to(self.device, torch.long).contiguous().view(-1)
        out = dict(nodes=0, ring_slots=0, ring_rows=0)
        N = self.num_nodes
        if not tgn.check_forget_args(N, ids.numel()):
            return out
        nb = int(_lib.lib().tgnx_tgn_forget_ws_bytes(ctypes.byref(tgn.TgnConfig(num_nodes=N))))
        if nb == 0:
            raise RuntimeError(f"tgnx_tgn_forget_ws_bytes: {_lib.lib().tgnx_last_error().decode()}")
        ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
        _lib.call("tgnx_ring_forget", _lib.ptr(self.neighbors), _lib.ptr(self.e_id), _lib.ptr(self.t), 0, 0, N,
                  self.size, _lib.ptr(ids), ids.numel(), _lib.ptr(ws), nb, _lib.stream(self.device))
        rec = ws[:64].view(torch.int64).tolist()      # (the call's kernels checked it too: a bad record stored nothing)
        if rec[4]:
            if bool(((ids < 0) | (ids >= N)).any()):
                raise ValueError(f"LastNeighborLoader.forget: node ids must be in [0, {N}); nothing was changed")
            raise RuntimeError(f"LastNeighborLoader.forget: {rec[4]} ring slots name a node outside [0, {N}); nothing "
                               "was changed")
        self.version += 1
        return {k: int(rec[i]) for i, k in enumerate(out)}

    def _workspace(self, q: int) -> torch.Tensor:
        if q > self._ws_q:
            q2 = max(q, 2 * max(self._ws_q, 0), 1024)
            nb = _lib.lib().tgnx_ring_sample_ws_bytes(self.num_nodes, q2)
            self._ws = torch.zeros(nb, dtype=torch.uint8, device=self.device)   # bitmap must start zeroed
            self._ws_q = q2
        return self._ws

    # neighbor_loader.py:26-50
    def __call__(self, n_id: torch.Tensor):
        n_id = torch.as_tensor(n_id).to(self.device, torch.long).contiguous()
        q = int(n_id.numel())
        K = self.size
        cap_n, cap_e = q * (1 + K), max(q * K, 1)
        out_nid = torch.empty(max(cap_n, 1), dtype=torch.long, device=self.device)
        out_ei = torch.empty(2 * cap_e, dtype=torch.long, device=self.device)
        out_eid = torch.empty(cap_e, dtype=torch.long, device=self.device)
        out_t = torch.empty(cap_e, dtype=torch.float, device=self.device)
        ws = self._workspace(q)
        _lib.call("tgnx_ring_sample", _lib.ptr(self.neighbors), _lib.ptr(self.e_id), _lib.ptr(self.t),
                  self.num_nodes, K, _lib.ptr(n_id), q, _lib.ptr(self._assoc), _lib.ptr(out_nid), _lib.ptr(out_ei),
                  _lib.ptr(out_eid), _lib.ptr(out_t), cap_n, cap_e, _lib.ptr(self._counts), _lib.ptr(ws),
                  ws.numel(), _lib.stream(self.device))
        M, E = self._counts.tolist()    # one D2H sync, like the reference's .unique()
        ei = out_ei.view(2, cap_e)[:, :E]
        return out_nid[:M], ei, out_eid[:E], out_t[:E]

    # neighbor_loader.py:52-104
    def insert(self, src: torch.Tensor, dst: torch.Tensor, t: torch.Tensor = None):
        src = torch.as_tensor(src).to(self.device, torch.long).contiguous()
        dst = torch.as_tensor(dst).to(self.device, torch.long).contiguous()
        t = torch.as_tensor(t).to(self.device, torch.float).contiguous()
        B = int(src.numel())
        cap = _lib.lib().tgnx_ring_insert_max_batch()
        if B > cap:
            raise RuntimeError(f"LastNeighborLoader.insert: batch {B} > {cap} supported by tgnx_ring_insert")
        _lib.call("tgnx_ring_insert", _lib.ptr(self.neighbors), _lib.ptr(self.e_id), _lib.ptr(self.t),
                  self.num_nodes, self.size, _lib.ptr(src), _lib.ptr(dst), _lib.ptr(t), B, self.cur_e_id,
                  _lib.ptr(self._assoc), _lib.stream(self.device))
        self.cur_e_id += B
        self.version += 1
