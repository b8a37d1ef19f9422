"""Inputs of the eviction tests' Take property (patrolhip.h "Choosing
idle_ns"), shared by tests/test_evict_abi.py (which checks them against the
oracle alone) and tests/test_evict.py (which reuses them on the GPU).

A bucket with state (added, taken, elapsed), created at `created`, is idle
for dt at NOW = created + elapsed + dt.  With dt >= per, a Take at NOW on it
and a Take at NOW on a bucket created afresh at NOW answer alike.  The rates
keep per >= freq > 0 (Rate.Interval = per / freq is then non-zero, so
Tokens(dt) >= Freq, bucket.go:132-148) and the states taken <= added (no
token debt), all values integers below 2^53 so that every sum is exact.
"""
SEC = 10**9
NOW = 1_700_000_000_000_000_000

# (freq, per, count)
RATES = [(100, SEC, 1), (5, SEC, 3), (3, 60 * SEC, 5), (7, 10, 7), (1, 1, 1), (100, SEC, 0)]
# (added, taken, elapsed)
STATES = [(100.0, 40.0, 5 * SEC), (0.0, 0.0, 0), (1000.0, 1000.0, 123456789),
          (float(2**52), float(2**52 - 3), 7), (5.0, 0.0, 3 * SEC)]


def dts(per):
    return (per, per + 1, 10 * per)


def buckets(rate):
    """-> [(name, added, taken, elapsed, created)] for one rate: every state
    at every dt, all idle for exactly dt at NOW."""
    _, per, _ = rate
    out = []
    for si, (a, t, e) in enumerate(STATES):
        for di, dt in enumerate(dts(per)):
            out.append((b"tp-%d-%d" % (si, di), a, t, e, NOW - e - dt))
    return out
