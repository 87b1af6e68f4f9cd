"""Test infrastructure: holders indexes and batches of any size, generated with
torch on a given device, and vectorised references of the index calls
(include/sdcas.h: remove, directory, add, match, peers) over the same tensors.
Nothing here imports the library: tests/test_index_scale_ref.py pins these
references on the CPU against the list references (tests/_chunk_holders_ref.py,
_chunk_index_ref.py, _chunk_peers_ref.py) before tests/test_gpu_index_scale.py
lets them judge a kernel at sizes those cannot reach.

Torch has little unsigned 64-bit arithmetic, so keys, values and file ids stay
below 2^63 and live in int64 tensors whose bytes are the uint64 the library
reads; a directory is an int32 tensor (its values are at most 2^30). Digests are
uint8 [n, 32] and are compared as memcmp does. All results are integers: every
comparison against the library is exact equality."""
import collections

import torch

T = 1 << 24                      # items from which the scan's third level has an index above 0
HIT, ADDED, SKIPPED = 1, 2, 4
EARLIER, ALL = 0, 1
MATCH_COUNTS = ("queries", "hits", "misses", "skipped")
ADD_COUNTS = ("queries", "hits", "added", "batch_duplicates", "entries_old", "entries_new")
REMOVE_COUNTS = ("entries_old", "removed", "entries_new", "values")
PEERS_COUNTS = ("files", "chunks", "common_chunks", "pairs", "edges", "files_with_peer", "overflow")
ZONE_STEP = 1 << 40              # what a value gains per `boundary` entries before its run
N_IDS = 64

Index = collections.namedtuple("Index", "keys digests values dir bits")
Batch = collections.namedtuple("Batch", "keys digests values")

_SIGN = -(1 << 63)


def _i64(x):
    """a 64-bit pattern as the Python int an int64 tensor takes"""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def _lsr(x, s):
    return (x >> s) & ((1 << (64 - s)) - 1)


def mix(x, salt=0):
    """splitmix64's finaliser over an int64 tensor (arithmetic modulo 2^64)"""
    x = x + _i64(0x9E3779B97F4A7C15 * (salt + 1))
    x = (x ^ _lsr(x, 30)) * _i64(0xBF58476D1CE4E5B9)
    x = (x ^ _lsr(x, 27)) * _i64(0x94D049BB133111EB)
    return x ^ _lsr(x, 31)


def dir_bits(n):
    """the recommended directory width: 0 below 8 entries, else min(28, ceil_log2(n) - 2)"""
    return 0 if n < 8 else min(28, (n - 1).bit_length() - 2)


def holder_ids(device, count=N_IDS):
    """`count` ascending ids below 2^40 that use more than 32 bits"""
    return (torch.arange(count, dtype=torch.int64, device=device) * 37 + 1000) * 0x1000193


# ---- order ---------------------------------------------------------------------------------

def order_words(digests):
    """uint8 [n, 32] -> int64 [n, 4] whose signed order, column after column, is
    the digests' memcmp order: each 8 bytes big-endian, the top bit flipped"""
    n = digests.shape[0]
    be = digests.reshape(n, 4, 8).flip(2).contiguous().view(torch.int64).reshape(n, 4)
    return be ^ _SIGN


def _lex_less(a, b):
    """rows of a before rows of b, column after column ([n, c] each)"""
    ne = a != b
    first = ne.int().argmax(1, keepdim=True)
    return (a.gather(1, first) < b.gather(1, first)).reshape(-1) & ne.any(1)


def lexsort(cols):
    """the stable order of rows by `cols` (int64 [n] each, the first decides
    first): rows that are equal keep their positions' order"""
    n = cols[0].shape[0]
    perm = torch.arange(n, dtype=torch.int64, device=cols[0].device)
    for col in reversed(cols):
        perm = perm[torch.sort(col[perm], stable=True).indices]
    return perm


def groups(cols):
    """-> (perm, head, gid): lexsort's order, whether a sorted place differs from
    the one before, and the number of the group of equal rows it belongs to"""
    perm = lexsort(cols)
    n = perm.shape[0]
    head = torch.zeros(n, dtype=torch.bool, device=perm.device)
    if n:
        head[0] = True
    for col in cols:
        s = col[perm]
        head[1:] |= s[1:] != s[:-1]
    return perm, head, torch.cumsum(head, 0) - 1


def _triple_cols(keys, digests, values):
    w = order_words(digests)
    return [keys, w[:, 0], w[:, 1], w[:, 2], w[:, 3], values]


def run_starts(keys, digests):
    """the entries of an index whose pair differs from the entry before"""
    n = keys.shape[0]
    head = torch.ones(n, dtype=torch.bool, device=keys.device)
    if n > 1:
        d = digests.view(torch.int64)
        head[1:] = (keys[1:] != keys[:-1]) | (d[1:] != d[:-1]).any(1)
    return torch.nonzero(head).reshape(-1)


# ---- the generator -------------------------------------------------------------------------

def directory(keys, n, bits):
    """dir[j] = the entries whose key's top `bits` bits are below j, as int32
    [2^bits + 1]; the keys are below 2^63, so the upper half holds n"""
    dev = keys.device
    if bits == 0:
        return torch.tensor([0, n], dtype=torch.int32, device=dev)
    half = 1 << (bits - 1)
    bounds = torch.arange(half, dtype=torch.int64, device=dev) << (64 - bits)
    low = torch.searchsorted(keys[:n].contiguous(), bounds)
    return torch.cat([low, torch.full((half + 1,), n, dtype=torch.int64, device=dev)]).to(torch.int32)


def gen_index(n, bits, device, salt=0, boundary=T, runs=(1, 8), ids=None, zone_step=ZONE_STEP):
    """A holders index of n entries: strictly ascending in (key, digest, value).
    One key in 16 carries two digests, in memcmp order; a pair is held by
    runs[0] .. runs[1] values, the number following the key; at least one run
    straddles every multiple of `boundary` below n (unless runs[1] is 1: then
    the index is a chunk index, every pair once). A digest is a mix of its
    key's number and the salt over all 32 bytes; a run's values are an
    ascending choice of `ids` plus zone_step for every `boundary` entries
    before the run (so that a set of removed values can keep different shares
    of different stretches of the index)."""
    ids = holder_ids(device) if ids is None else ids
    n_ids = ids.shape[0]
    rmin, rmax = runs
    assert 1 <= rmin <= rmax < n_ids
    if n == 0:
        z = torch.zeros(0, dtype=torch.int64, device=device)
        return Index(z, torch.zeros((0, 32), dtype=torch.uint8, device=device), z.clone(), directory(z, 0, bits), bits)
    # enough key numbers: surely when every run has rmin holders, else 5 % and 64 keys above the expected need
    n_q = n // rmin + 8 if rmin == rmax else int(n / (1.0625 * (rmin + rmax) / 2) * 1.05) + 64
    q_all = torch.arange(n_q, dtype=torch.int64, device=device)
    per_key = 1 + ((mix(q_all, salt + 11) & 15) == 0).to(torch.int64)
    pair_q = torch.repeat_interleave(q_all, per_key)
    slot = torch.arange(pair_q.shape[0], dtype=torch.int64, device=device) - (torch.cumsum(per_key, 0) - per_key)[pair_q]
    run = rmin + _lsr(mix(pair_q * 2 + slot, salt + 12), 8) % (rmax - rmin + 1)
    start = torch.cumsum(run, 0) - run
    for b in range(boundary, n if rmax > 1 else 0, boundary):  # over the boundaries, not the entries
        p = int(torch.searchsorted(start, torch.tensor([b], device=device), right=True)) - 1
        if int(start[p]) == b:  # a run begins here: the run before takes one more holder
            run[p - 1] += 1
            start = torch.cumsum(run, 0) - run
    total = int(start[-1] + run[-1])
    assert total >= n, "the generator made too few pairs"
    n_pairs = int((start < n).sum())
    pair_q, slot, run, start = pair_q[:n_pairs], slot[:n_pairs], run[:n_pairs].clone(), start[:n_pairs]
    run[-1] = n - start[-1]
    # keys: the used key numbers spread over [0, 2^63)
    n_keys = int(pair_q[-1]) + 1
    step = min((1 << 63) // n_keys, 1 << 62)
    pair_key = pair_q * step + _lsr(mix(pair_q, salt + 13), 2) % step
    # digests: two candidates per key number; a key with two takes them in memcmp order
    cand = [torch.stack([mix(pair_q * 8 + j, salt + 14 + 7 * c) for j in range(4)], 1) for c in range(2)]
    a_first = _lex_less(order_words(cand[0].view(torch.uint8).reshape(-1, 32)),
                        order_words(cand[1].view(torch.uint8).reshape(-1, 32)))
    use_a = torch.where(per_key[pair_q] == 2, (slot == 0) == a_first, torch.ones_like(a_first))
    pair_words = torch.where(use_a[:, None], cand[0], cand[1])
    # entries
    ent = torch.repeat_interleave(torch.arange(n_pairs, dtype=torch.int64, device=device), run)
    j = torch.arange(n, dtype=torch.int64, device=device) - start[ent]
    r = run[ent]
    pick = (j * n_ids) // r + _lsr(mix(ent * 64 + j, salt + 15), 4) % (n_ids // r)
    keys = pair_key[ent]
    values = ids[pick] + zone_step * (start[ent] // boundary)
    digests = pair_words[ent].contiguous().view(torch.uint8).reshape(n, 32)
    return Index(keys, digests, values, directory(keys, n, bits), bits)


def gen_batch(old, m, device, salt=1, distinct_pairs=False):
    """A batch of m triples for an add to `old`, in a fixed shuffled order:
    a quarter are old entries spread over the whole index (hits; an entry more
    than once when `old` is smaller than that), a quarter are later copies of
    new triples, the rest are new triples of an index generated with another
    salt. distinct_pairs (for the chunk index's add): no copies, one value per
    new pair, an old entry at most once; `old` must hold each pair once."""
    n_old = old.keys.shape[0]
    n_hits = min(m // 4, n_old) if distinct_pairs else m // 4 if n_old else 0  # an old entry may hit twice
    n_dup = 0 if distinct_pairs else m // 4
    n_new = m - n_hits - n_dup
    new = gen_index(n_new, 0, device, salt=salt, boundary=max(m, 1), runs=(1, 1) if distinct_pairs else (1, 8))
    at = (torch.arange(n_hits, dtype=torch.int64, device=device) * n_old) // max(n_hits, 1)
    again = (torch.arange(n_dup, dtype=torch.int64, device=device) * 7919) % max(n_new, 1)
    order = torch.sort(mix(torch.arange(m, dtype=torch.int64, device=device), salt + 21)).indices
    return Batch(*(torch.cat([fresh, stored[at], fresh[again]])[order].contiguous()
                   for fresh, stored in zip(new[:3], old[:3])))


def gen_queries(index, m, device, salt=2):
    """m queries for a match in a fixed shuffled order: a quarter miss (pairs of
    an index generated with another salt), the hits are runs spread evenly over
    the whole index, the first and the last run among them -> (keys, digests)"""
    starts = run_starts(index.keys, index.digests)
    n_runs = starts.shape[0]
    n_miss = m // 4 if n_runs else m
    n_hit = m - n_miss
    which = (torch.arange(n_hit, dtype=torch.int64, device=device) * (n_runs - 1)) // max(n_hit - 1, 1)
    at = starts[which]
    other = gen_index(n_miss, 0, device, salt=salt, boundary=max(m, 1), runs=(1, 1))
    order = torch.sort(mix(torch.arange(m, dtype=torch.int64, device=device), salt + 21)).indices
    return (torch.cat([index.keys[at], other.keys])[order].contiguous(),
            torch.cat([index.digests[at], other.digests])[order].contiguous())


def gen_chunks(index, m, n_files, device, hit_one_in=1, hit_all_from=None, len_bits=16, salt=3):
    """A batch of m chunks for the peers -> (keys, digests, chunk_file int32,
    chunk_len, file_ids). Chunk c belongs to file c % n_files; one chunk in
    hit_one_in, and every chunk from hit_all_from on, is a pair of the index
    (any run, by a mix of c), the others are pairs of their own; the lengths are
    below 2^len_bits. One file in 8 has a holder's id (it is its own holder in
    some runs and EARLIER mode counts only a part of a run); the others have
    ids above every holder's."""
    starts = run_starts(index.keys, index.digests)
    c = torch.arange(m, dtype=torch.int64, device=device)
    hit = _lsr(mix(c, salt + 31), 3) % hit_one_in == 0
    if hit_all_from is not None:
        hit |= c >= hit_all_from
    at = starts[_lsr(mix(c, salt + 32), 1) % starts.shape[0]]
    own = torch.stack([mix(c * 8 + j, salt + 33) for j in range(4)], 1).view(torch.uint8).reshape(m, 32)
    keys = torch.where(hit, index.keys[at], _lsr(mix(c, salt + 34), 1))
    digests = torch.where(hit[:, None], index.digests[at], own)
    f = torch.arange(n_files, dtype=torch.int64, device=device)
    ids = holder_ids(device)
    file_ids = torch.where(f % 8 == 0, ids[(f // 8) % ids.shape[0]], (1 << 50) + f)
    return keys, digests, (c % n_files).to(torch.int32), _lsr(mix(c, salt + 35), 64 - len_bits), file_ids


# ---- the references --------------------------------------------------------------------------

def remove(index, removed, bits_new):
    """-> (keep mask, Index of the entries whose value is not in `removed`, counts)"""
    keep = ~torch.isin(index.values, removed)
    k, d, v = index.keys[keep], index.digests[keep], index.values[keep]
    n, e = index.keys.shape[0], k.shape[0]
    return keep, Index(k, d, v, directory(k, e, bits_new), bits_new), dict(
        entries_old=n, removed=n - e, entries_new=e, values=removed.shape[0])


def add(old, batch, bits_new):
    """The holders add, read per triple -> (Index, pos int64[m], flags uint8[m],
    counts, fresh: per place of the batch's own triple order, whether a new
    triple's first copy stands there). One stable sort of old ++ batch by the
    triple: a group of equal triples holds at most one old entry, which comes
    first, then the batch's copies by position."""
    n_old, m = old.keys.shape[0], batch.keys.shape[0]
    keys, dig, vals = (torch.cat([a, b]) for a, b in zip(old[:3], batch))
    perm, head, gid = groups(_triple_cols(keys, dig, vals))
    firsts = perm[head]                                     # the group's first row: old if any is
    is_batch = perm >= n_old
    stored = (firsts < n_old)[gid]                          # by sorted place: the group has an old entry
    flag_sorted = torch.where(stored, HIT, torch.where(head, ADDED, 0)).to(torch.uint8)
    c = perm[is_batch] - n_old
    pos = torch.empty(m, dtype=torch.int64, device=keys.device)
    flags = torch.empty(m, dtype=torch.uint8, device=keys.device)
    pos[c], flags[c] = gid[is_batch], flag_sorted[is_batch]
    e = firsts.shape[0]
    k = keys[firsts]
    hits, added = int((flags == HIT).sum()), int((flags == ADDED).sum())
    counts = dict(queries=m, hits=hits, added=added, batch_duplicates=m - hits - added, entries_old=n_old,
                  entries_new=e)
    return Index(k, dig[firsts], vals[firsts], directory(k, e, bits_new), bits_new), pos, flags, counts, \
        flag_sorted[is_batch] == ADDED


def distinct_pairs(old, batch):
    """The precondition under which the chunk index's add and the holders
    index's add are defined to agree: the batch's pairs are distinct, and
    old ++ batch holds as many distinct pairs as distinct triples (so `old`
    holds each pair once and a batch pair that is stored carries the stored
    value)."""
    own = _triple_cols(*batch)[:5]
    cols = _triple_cols(*(torch.cat([a, b]) for a, b in zip(old[:3], batch)))
    return (int(groups(own)[1].sum()) == batch.keys.shape[0]
            and int(groups(cols[:5])[1].sum()) == int(groups(cols)[1].sum()))


def match(index, keys, digests):
    """-> (pos: the pair's first entry or -1, value: the lowest holder or 0,
    holders int32: the entries with the pair, counts), by a sort of the run
    starts' pairs ++ the queries"""
    n, m = index.keys.shape[0], keys.shape[0]
    dev = keys.device
    starts = run_starts(index.keys, index.digests)
    s = starts.shape[0]
    length = torch.diff(starts, append=torch.tensor([n], dtype=torch.int64, device=dev))
    w = order_words(torch.cat([index.digests[starts], digests]))
    perm, head, gid = groups([torch.cat([index.keys[starts], keys])] + [w[:, j] for j in range(4)])
    first = perm[head][gid]                                 # by sorted place: the group's first row
    q = perm >= s
    c, run = perm[q] - s, first[q]
    hit = run < s
    run = run.clamp(max=max(s - 1, 0))
    pos = torch.full((m,), -1, dtype=torch.int64, device=dev)
    value = torch.zeros(m, dtype=torch.int64, device=dev)
    holders = torch.zeros(m, dtype=torch.int32, device=dev)
    if s:
        pos[c] = torch.where(hit, starts[run], -1)
        value[c] = torch.where(hit, index.values[starts[run]], 0)
        holders[c] = torch.where(hit, length[run], 0).to(torch.int32)
    hits = int(hit.sum()) if s else 0
    return pos, value, holders, dict(queries=m, hits=hits, misses=m - hits, skipped=0)


def peers(index, keys, digests, chunk_file, chunk_len, file_ids, k, max_holders, mode, max_pairs, ids):
    """The chunk peers with every chunk valid, over a dense [n_files, len(ids)]
    matrix: every value of the index is one of `ids` (ascending); chunk_file is
    int32, chunk_len int64 with every sum below 2^63. -> dict of peer_count
    int32 [n], peers / peer_bytes int64 [n, k], shared / unique / common int64
    [n], counts, and for the tests' own conditions pairs_per_file int64 [n],
    edge_bytes int64 [n, len(ids)] and counted int64 [m] (a chunk's counted
    holders, 0 when it is common or takes no part)."""
    dev = keys.device
    n_files, n_ids, n = file_ids.shape[0], ids.shape[0], index.keys.shape[0]
    pos, _, holders, _ = match(index, keys, digests)
    part = chunk_file.to(torch.int64) < n_files
    f_all = chunk_file.to(torch.int64).clamp(max=max(n_files - 1, 0))
    # the runs of the chunks that hit, as a [hits, longest run] matrix of values
    h = torch.nonzero(part & (holders > 0)).reshape(-1)
    width = int(holders.max()) if holders.numel() else 0
    col = torch.arange(max(width, 1), dtype=torch.int64, device=dev)[None, :]
    inside = col < holders[h].to(torch.int64)[:, None]
    vals = index.values[(pos[h][:, None] + col).clamp(max=max(n - 1, 0))] if n else torch.zeros_like(inside, dtype=torch.int64)
    fid = file_ids[f_all[h]][:, None]
    counted = inside & (vals < fid if mode == EARLIER else vals != fid)
    cnt_h = counted.sum(1)
    cnt = torch.zeros(keys.shape[0], dtype=torch.int64, device=dev)
    cnt[h] = cnt_h
    is_common = part & (cnt > max_holders)
    is_shared = part & (cnt > 0) & ~is_common
    is_unique = part & (cnt == 0)

    def per_file(mask):
        return torch.zeros(n_files, dtype=torch.int64, device=dev).index_add_(0, f_all[mask], chunk_len[mask])

    shared, unique, common = per_file(is_shared), per_file(is_unique), per_file(is_common)
    scoring = counted & ~is_common[h][:, None]
    rows = f_all[h][:, None].expand_as(scoring)[scoring]
    where = torch.searchsorted(ids, vals[scoring])
    assert bool((ids[where.clamp(max=n_ids - 1)] == vals[scoring]).all()), "a holder outside `ids`"
    lens = chunk_len[h][:, None].expand_as(scoring)[scoring]
    score = torch.zeros((n_files, n_ids), dtype=torch.int64, device=dev).index_put_((rows, where), lens, accumulate=True)
    times = torch.zeros((n_files, n_ids), dtype=torch.int64, device=dev).index_put_(
        (rows, where), torch.ones_like(lens), accumulate=True)
    present = times > 0
    pairs = int(times.sum())
    over = pairs > max_pairs
    counts = dict(files=n_files, chunks=int(part.sum()), common_chunks=int(is_common.sum()), pairs=pairs,
                  edges=0 if over else int(present.sum()), files_with_peer=0 if over else int(present.any(1).sum()),
                  overflow=int(over))
    peer_count = torch.zeros(n_files, dtype=torch.int32, device=dev)
    who = torch.zeros((n_files, k), dtype=torch.int64, device=dev)
    how = torch.zeros((n_files, k), dtype=torch.int64, device=dev)
    if not over and n_files:
        # bytes descending; the columns are in id order and the sort is stable
        order = torch.sort(torch.where(present, score, -1), dim=1, descending=True, stable=True).indices
        kk = min(k, n_ids)
        n_peers = present.sum(1)
        top = torch.arange(kk, dtype=torch.int64, device=dev)[None, :] < n_peers[:, None]
        who[:, :kk] = torch.where(top, ids[order[:, :kk]], 0)
        how[:, :kk] = torch.where(top, score.gather(1, order[:, :kk]), 0)
        peer_count = n_peers.clamp(max=k).to(torch.int32)
    return {"peer_count": peer_count, "peers": who, "peer_bytes": how, "shared": shared, "unique": unique,
            "common": common, "counts": counts, "pairs_per_file": times.sum(1), "edge_bytes": score,
            "counted": torch.where(is_common, 0, cnt)}
