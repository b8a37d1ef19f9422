"""The change set of a tracking handle (include/patrolhip.h "Change set") as
plain Python over the oracle, built on tests/_egress_cases.py and shared by
tests/test_changes_abi.py (no GPU) and tests/test_changes.py.

A Model follows one oracle repo through the op batches applied since the last
drain, optionally with evictions between them:
  - the requests are the names whose creating op was a TAKE;
  - the states are the oracle's current dump for every name a TAKE / UPSERT
    touched, minus zero states, names over 231 bytes and evicted names.
"""
from __future__ import annotations

import numpy as np

from tests import _egress_cases as EC
from tests._egress_cases import TAKE, RECEIVE, UPSERT, CREATED, MAX_NAME  # noqa: F401


class Model:
    def __init__(self, oracle):
        self.o = oracle
        self.gone = set()      # names evicted from the table under test (the oracle keeps them)
        self.req = {}          # name -> None, in marking order (a dict as an ordered set)
        self.touched = set()

    def batch(self, ops):
        """An ordered batch that marks (phip_apply_mixed and what runs through
        it) -> the oracle's results."""
        ref = EC.call(self.o, ops)
        first = {}
        for i, nm in enumerate(ops["names"]):
            first.setdefault(nm, i)
            if ops["kind"][i] in (TAKE, UPSERT):
                self.touched.add(nm)
        for nm, i in first.items():
            if ops["kind"][i] == TAKE and (int(ref["status"][i]) & CREATED):
                self.req[nm] = None
        return ref

    def unmarked(self, ops):
        """A batch that changes the table and marks nothing (the egress call)."""
        return EC.call(self.o, ops)

    def receive_soa(self, names, a, t, e, now):
        """Received merges are never rebroadcast: the oracle only."""
        return self.o.receive_soa(names, a, t, e, now)

    def evict(self, names):
        """These buckets left the table under test: their marks go with them."""
        for nm in names:
            self.gone.add(nm)
            self.req.pop(nm, None)
            self.touched.discard(nm)

    def expected(self):
        """-> (request datagrams by name, state datagrams by name) of a full drain."""
        dump = self.o.dump()
        req = {nm: EC.request(nm) for nm in self.req if len(nm) <= MAX_NAME}
        st = {}
        for nm in self.touched:
            a, t, e = dump[nm][:3]
            if len(nm) <= MAX_NAME and not EC.is_zero(a, t, e):
                st[nm] = EC.marshal(nm, a, t, e)
        return req, st

    def pending(self):
        """Marks set: every request and every touched name, left-out ones included."""
        return len(self.req) + len(self.touched)

    def drained(self):
        self.req.clear()
        self.touched.clear()

    def datagrams(self):
        """A full drain in the order it leaves: requests, then states."""
        req, st = self.expected()
        return list(req.values()) + list(st.values())


def split(ops, cuts):
    """An op stream cut into consecutive batches at the given indices."""
    n = len(ops["names"])
    edges = [0] + sorted(cuts) + [n]
    out = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        b = {k: (v[lo:hi] if k == "names" else np.ascontiguousarray(v[lo:hi])) for k, v in ops.items()}
        out.append(b)
    return [b for b in out if len(b["names"])]
