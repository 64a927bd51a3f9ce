"""World N in ONE process, one rank after the other -- test helper for the synchronised BatchNorm nodes (train_nodes._MaskedBNActFn, pfn_train.FusedPFNTrain).

Both nodes reach their collective through dist_utils.all_reduce_sum(t, group), looked up at call time, and hand on whatever object enable_sync() was
given.  Threads cannot stand in for ranks: the backward nodes of every caller run on the device's one autograd worker thread, so a barrier inside
a node would deadlock.  Replay instead:

    rp = Replay(world)
    results = rp.run(fn)                     # fn(rank, token) -> anything; token goes to enable_sync(process_group=token)

A pass calls fn(rank, token) for rank 0 .. world - 1 in turn, with dist_utils.all_reduce_sum replaced.  fn builds its state afresh in every call (a
deep copy of the module, fresh leaf tensors).  The k-th collective of a rank records a float64 clone of its local tensor; if the global sum of index
k is known from an earlier pass it is copied into the tensor, otherwise the tensor stays local and the pass is provisional.  After a provisional
pass the sum over the ranks at the first unknown index is stored (that index's contributions depended on known sums only, so they are exact) and
the pass is repeated: with L collectives per rank pass L + 1 is exact, and its results are returned.

Asserted in every pass: every rank issued the same number of collectives with the same shapes and dtypes (a rank that skips one would hang a real
run), every collective carried the token of the rank that is running, and the contributions at already-known indices are bit-identical to those of
the pass before (a node whose sums change from call to call cannot be replayed -- nor reproduced)."""
import torch


class ReplayError(AssertionError):
    pass


class _Token:
    """Stands in for a process group: one per rank."""

    def __init__(self, replay, rank):
        self.replay, self.rank = replay, rank

    def __repr__(self):
        return f"<replay rank {self.rank} of {self.replay.world}>"


class Replay:
    def __init__(self, world):
        assert world >= 1
        self.world = world
        self.tokens = [_Token(self, r) for r in range(world)]
        self.known = []          # global sums (float64) by collective index
        self.passes = 0
        self._rank = None
        self._log = self._dtypes = None

    # the replacement of dist_utils.all_reduce_sum
    def _all_reduce_sum(self, t, group=None):
        if self._rank is None:
            raise ReplayError("collective outside a replay pass")
        if group is not self.tokens[self._rank]:
            raise ReplayError(f"rank {self._rank}: the collective carries {group!r}, not the group given to enable_sync")
        log = self._log[self._rank]
        k = len(log)
        log.append(t.detach().to(torch.float64).clone())
        self._dtypes[self._rank].append(t.dtype)
        if k < len(self.known):
            g = self.known[k]
            if g.shape != t.shape:
                raise ReplayError(f"rank {self._rank}, collective {k}: shape {tuple(t.shape)}, the earlier passes had {tuple(g.shape)}")
            with torch.no_grad():
                t.copy_(g.to(device=t.device, dtype=t.dtype))
        return t

    def _one_pass(self, fn):
        from pillarnext_amd import dist_utils

        self._log = [[] for _ in range(self.world)]
        self._dtypes = [[] for _ in range(self.world)]
        old = dist_utils.all_reduce_sum
        dist_utils.all_reduce_sum = self._all_reduce_sum
        try:
            out = []
            for r in range(self.world):
                self._rank = r
                out.append(fn(r, self.tokens[r]))
        finally:
            self._rank = None
            dist_utils.all_reduce_sum = old
        return out

    def run(self, fn, max_passes=16):
        prev = None
        while True:
            n_known = len(self.known)
            out = self._one_pass(fn)
            self.passes += 1
            log = self._log
            counts = [len(l) for l in log]
            if len(set(counts)) != 1:
                raise ReplayError(f"pass {self.passes}: the ranks issued {counts} collectives -- a real run would hang")
            for k in range(counts[0]):
                sig = [(tuple(l[k].shape), str(l[k].device)) for l in log]
                if len(set(sig)) != 1:
                    raise ReplayError(f"pass {self.passes}, collective {k}: the ranks disagree on the tensor: {sig}")
            if any(d != self._dtypes[0] for d in self._dtypes):
                raise ReplayError(f"pass {self.passes}: the ranks disagree on a collective's dtype: {self._dtypes}")
            if prev is not None:
                for r in range(self.world):
                    for k in range(min(n_known, len(prev[r]), counts[0])):
                        if not torch.equal(prev[r][k], log[r][k]):
                            raise ReplayError(f"pass {self.passes}, rank {r}, collective {k}: the contribution differs from the pass before "
                                              f"although every sum it depends on was the same (max |diff| {float((prev[r][k] - log[r][k]).abs().max()):.3e})")
            if counts[0] < n_known:
                raise ReplayError(f"pass {self.passes}: {counts[0]} collectives, the passes before had at least {n_known}")
            if counts[0] == n_known:
                return out
            if self.passes >= max_passes:
                raise ReplayError(f"no exact pass after {self.passes} passes")
            self.known.append(torch.stack([l[n_known] for l in log]).sum(0))
            prev = log
