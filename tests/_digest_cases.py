"""The partition digest's model (patrolhip.h "Partition digests"), shared by
tests/test_digest_abi.py (which checks it against the host helpers and the
oracle alone) and tests/test_digest.py (which holds the GPU to it).

From the rows of a dump, {name: (added bits, taken bits, elapsed, created)}:
  tag(name)      FNV-1a 64 of the name, masked to debug_tag_bits, 0 stored as 1
  part(tag, k)   k ? fmix(tag) >> (64 - k) : 0, fmix = murmur3's finaliser
  rec_hash       fmix chain over tag, canon(added), canon(taken), elapsed,
                 canon(-0.0 bits) = 0
  digest(rows,k) per partition the sum mod 2^64 of rec_hash and the count of
                 the covered rows: those the unfiltered sweep exports
                 (tests/_sweep_cases.py: not a zero state, name <= 231 bytes)
  exported(...)  the sweep's model restricted to a partition mask
  window(...)    the slots one filtered call reads at most
"""
from tests import _sweep_cases as SC

M64 = (1 << 64) - 1
SIGN = 1 << 63
GOLDEN = 0x9E3779B97F4A7C15
MAX_LOG2 = 20


def fnv1a64(name):
    h = 0xcbf29ce484222325
    for c in name:
        h = ((h ^ c) * 0x100000001b3) & M64
    return h


def fmix(x):
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def tag(name, tag_bits=0):
    h = fnv1a64(name)
    if 0 < tag_bits < 64:
        h &= (1 << tag_bits) - 1
    return h or 1


def part(t, k):
    return fmix(t) >> (64 - k) if k else 0


def canon(bits):
    return 0 if bits == SIGN else bits


def rec_hash(t, a_bits, t_bits, elapsed):
    h = fmix((t + GOLDEN) & M64)
    h = fmix(h ^ canon(a_bits))
    h = fmix(h ^ canon(t_bits))
    return fmix(h ^ (elapsed & M64))


def covered(name, a, t, e):
    return len(name) <= SC.MAX_NAME and not SC.is_zero(a, t, e)


def digest(rows, k, tag_bits=0):
    """-> (sums, counts, records, bytes): two lists of 2^k ints and the totals."""
    sums, counts = [0] * (1 << k), [0] * (1 << k)
    nbytes = 0
    for name, (a, t, e, _c) in rows.items():
        if not covered(name, a, t, e):
            continue
        tg = tag(name, tag_bits)
        p = part(tg, k)
        sums[p] = (sums[p] + rec_hash(tg, a, t, e)) & M64
        counts[p] += 1
        nbytes += SC.FIXED + len(name)
    return sums, counts, sum(counts), nbytes


def diff(da, db):
    """Partitions at which two model digests (sums, counts, ...) differ."""
    return {p for p in range(len(da[0])) if da[0][p] != db[0][p] or da[1][p] != db[1][p]}


def mask_words(parts, k):
    """A set of partitions as the uint64 words of the C mask."""
    words = [0] * max(1, (1 << k) // 64)
    for p in parts:
        words[p >> 6] |= 1 << (p & 63)
    return words


def in_mask(mask, p):
    return (int(mask[p >> 6]) >> (p & 63)) & 1 == 1


def exported(rows, k, mask, now=0, idle_ns=0, tag_bits=0):
    """SC.exported restricted to the partitions whose bit is set in `mask`
    (uint64 words)."""
    out = SC.exported(rows, now, idle_ns)
    return {nm: dg for nm, dg in out.items() if in_mask(mask, part(tag(nm, tag_bits), k))}


def window(max_msgs, k, m):
    """W of a filtered call with m of the 2^k partitions asked for (m > 0)."""
    w = max(4 * max_msgs * -(-(1 << k) // m), SC.TILE)
    return (w + SC.TILE - 1) // SC.TILE * SC.TILE


def nan_parts(rows_list, k, tag_bits=0):
    """Partitions holding a covered bucket with a NaN field on any side."""
    def is_nan(b):
        return (b & ~SIGN) > 0x7FF0000000000000
    out = set()
    for rows in rows_list:
        for name, (a, t, e, _c) in rows.items():
            if covered(name, a, t, e) and (is_nan(a) or is_nan(t)):
                out.add(part(tag(name, tag_bits), k))
    return out
