"""csrc/tile_sort.h through dgr_debug_tile_sort: every sorting routine of the binning kernels, called as they call it, against
np.sort of the same 64-bit keys (depth bits << 32 | id).  The keys of a list are unique, so the sorted order is unique and
every comparison is array_equal.

What decides a routine's path is the list length and the keys' depth bits (include/dgr_hip.h names the modes):
  * sort_tile_in_wave takes the register network of 1, 2, 4, 8 or 16 words per lane at n <= 64, 128, 256, 512, 1024;
  * the network orders 32-bit words: 22 bits of (depth bits - the list's smallest) << clz(the list's depth range) | the entry's
    position in the unsorted list.  Entries that agree in the 22 bits are put right by a fix-up on the full keys (sort_wave_trunc:
    any_tie, final_position); sorted position p sits in register p % NCH of lane p / NCH, and the tie test looks at register
    neighbours, at the neighbouring lane's last register, and must not take the padding words (all ones) behind position n - 1
    for run-mates of an entry whose own word has all prefix bits set;
  * lists above 1024 entries are sorted in parts of 512 (the last one may hold a single entry) and merged by rank;
  * wg_sort_global pads to a power of two only in its index arithmetic (`j < n`).
One launch per mode holds every list of that mode.  (The last test needs no GPU: it checks the lists themselves.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from dgr_amd import _capi

WAVE, PART, MERGE, GLOBAL, GLOBAL_256 = range(5)   # DGR_TILE_SORT_*
WAVE_LENGTHS = (1, 2, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024)
LENGTHS = {WAVE: WAVE_LENGTHS, PART: tuple(n for n in WAVE_LENGTHS if n <= 512), MERGE: (1025, 1536, 1537, 2049, 6143, 6144),
           GLOBAL: (1, 2, 3, 2048, 2049, 6145, 8193), GLOBAL_256: (1, 2, 3, 2048, 2049, 6145, 8193)}
RUNS = (2, 16, 17, 65)
ONE = np.float32(1.0).view(np.uint32)


def words_per_lane(mode, n):
    """NCH of the network that sorts a list (a part) of n entries"""
    if mode != WAVE:
        return 8
    return 1 if n <= 64 else 2 if n <= 128 else 4 if n <= 256 else 8 if n <= 512 else 16


def unique_ids(rng, n, top=False):
    ids = rng.permutation(4 * n)[:n].astype(np.uint64) * 977 + rng.integers(0, 977)
    return (np.uint64(0xFFFFFFFF) - ids) if top else ids


def keys_of(depth_bits, ids):
    k = (np.asarray(depth_bits, np.uint64) << np.uint64(32)) | np.asarray(ids, np.uint64)
    assert np.unique(k).size == k.size
    return k


def with_ends(rng, n, lo, hi):
    """n depth words in [lo, hi], both ends present (n >= 2; one entry: lo)"""
    d = rng.integers(lo, hi + 1, n, dtype=np.uint64)
    if n >= 2:
        i, j = rng.permutation(n)[:2]
        d[i], d[j] = lo, hi
    else:
        d[:] = lo
    return d


def run_list(rng, n, L, start):
    """A list whose sorted positions start .. start + L - 1 share their 22-bit prefix: the smallest depth word is 0 and the
    largest has its top bit set, so the prefix of a word is its upper 22 bits.  The run's members differ in the low ten bits or
    in the id alone; a run that ends at n - 1 has the largest prefix (all ones: its words look like padding but for the slot)."""
    groups = n - L + 1
    top = (1 << 22) - 1
    if groups == 1:
        prefix = np.array([top], np.uint64)
    else:
        inner = np.cumsum(rng.integers(1, (top - 1) // groups, groups - 2)).astype(np.uint64)   # ascending, 0 < .. < top
        prefix = np.concatenate([[0], inner, [top]]).astype(np.uint64)
    which = np.concatenate([np.arange(start), np.full(L, start), np.arange(start + 1, groups)]).astype(np.int64)
    low = rng.integers(0, 1024, n).astype(np.uint64)
    low[start:start + L] = rng.integers(0, 4, L)
    d = (prefix[which] << np.uint64(10)) | low
    if groups > 1:
        d[0] = 0   # (sorted position 0 has prefix 0, inside the run or not)
    k = keys_of(d, unique_ids(rng, n))
    return k[rng.permutation(n)]


def families(mode, n, rng):
    """[(name, keys in their unsorted order)] of one length"""
    nch = words_per_lane(mode, n)
    octave = ONE + rng.integers(0, 1 << 23, n, dtype=np.uint64)
    out = [("octave", keys_of(octave, unique_ids(rng, n))),
           ("one depth", keys_of(np.full(n, ONE + 12345), unique_ids(rng, n, top=True))),
           ("two depths", keys_of(ONE + 77 * rng.integers(0, 2, n, dtype=np.uint64), unique_ids(rng, n))),
           ("64 neighbours", keys_of(ONE + (1 << 22) + rng.integers(0, 64, n, dtype=np.uint64), unique_ids(rng, n))),
           ("full span", keys_of(with_ends(rng, n, 0, 0xFFFFFFFF), unique_ids(rng, n)))]
    for k in (10, 22, 31):
        for r in ((1 << k) - 1, 1 << k):
            base = int(ONE) if k < 31 else 5
            out.append((f"range {r}", keys_of(with_ends(rng, n, base, base + r), unique_ids(rng, n))))
    asc = np.sort(keys_of(octave, unique_ids(rng, n)))
    out += [("ascending", asc), ("descending", asc[::-1].copy())]
    # the largest prefix together with the largest slot: the LAST entry of the unsorted list has the largest depth word
    d = with_ends(rng, n, 0, 0xFFFFFFFF)
    d[d == 0xFFFFFFFF] = 0xFFFFFFFE
    d[n - 1] = 0xFFFFFFFF
    if n > 1:
        d[0] = 0
    out.append(("largest word last", keys_of(d, unique_ids(rng, n))))
    for L in RUNS:
        if L > n:
            continue
        starts = {"end": n - L}
        lane = nch * max(1, (n // 2) // nch) - 1      # positions lane, lane + 1 lie in neighbouring lanes
        if lane >= 0 and lane + L <= n:
            starts["lane boundary"] = lane
        reg = nch * ((n // 3) // nch)                  # positions reg, reg + 1 are registers 0 and 1 of one lane
        if nch > 1 and reg + L <= n:
            starts["register boundary"] = reg
        for where, s in starts.items():
            out.append((f"run of {L} at {s} ({where})", run_list(rng, n, L, s)))
    return out


_cases = {}


def cases(mode):
    """[(name, keys)] of a mode, built once"""
    if mode not in _cases:
        rng = np.random.default_rng(100 + mode)
        _cases[mode] = [(f"n={n} {name}", k) for n in LENGTHS[mode] for name, k in families(mode, n, rng)]
    return _cases[mode]


def device_sort(mode, lists):
    """what the mode writes, per list: ids (WAVE, MERGE) or keys"""
    lib = _capi.load()
    dev = torch.device("cuda:0")
    offsets = np.concatenate([[0], np.cumsum([len(k) for k in lists])]).astype(np.int32)
    keys = torch.from_numpy(np.concatenate(lists).view(np.int64)).to(dev)
    ids_out = mode in (WAVE, MERGE)
    out = torch.full((keys.numel(),), -1, dtype=torch.int32 if ids_out else torch.int64, device=dev)
    rc = lib.dgr_debug_tile_sort(_capi.stream_handle(), mode, len(lists), keys.data_ptr(),
                                 offsets.ctypes.data_as(C.POINTER(C.c_int)), out.data_ptr() if ids_out else None,
                                 None if ids_out else out.data_ptr())
    assert rc == 0, _capi.last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32 if ids_out else np.uint64)
    return [got[a:b] for a, b in zip(offsets[:-1], offsets[1:])]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [WAVE, PART, MERGE, GLOBAL, GLOBAL_256],
                         ids=["sort_tile_in_wave", "sort_list_part", "parts_and_merge", "wg_sort_global_512", "wg_sort_global_256"])
def test_every_list_comes_back_in_key_order(mode):
    named = cases(mode)
    got = device_sort(mode, [k for _, k in named])
    wrong = []
    for (name, k), g in zip(named, got):
        want = np.sort(k)
        if mode in (WAVE, MERGE):
            want = (want & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        if not np.array_equal(g, want):
            wrong.append((name, int(np.count_nonzero(g != want))))
    assert not wrong, (len(wrong), wrong[:12])


def test_the_cases_hold_what_the_docstring_says():
    """the run lists really have their run where the network's layout puts a boundary (checked on the host, with the word the
    kernel forms), and every family is present at every length"""
    for mode in (WAVE, PART):
        for name, k in cases(mode):
            if " run of " not in name:
                continue
            n = k.size
            L, s = int(name.split(" run of ")[1].split()[0]), int(name.split(" at ")[1].split()[0])
            d = (np.sort(k) >> np.uint64(32)).astype(np.int64)
            if n > L:
                assert d[0] == 0 and d[-1] >= 1 << 31, name     # shift 0, smallest 0: the prefix is the word's upper 22 bits
                p = d >> 10
                assert np.all(p[s:s + L] == p[s]), name
                assert (s == 0 or p[s - 1] != p[s]) and (s + L == n or p[s + L] != p[s]), name
            if "(end)" in name and n > L:
                assert d[-1] >> 10 == (1 << 22) - 1, name
    per_length = {n: sum(1 for name, _ in cases(WAVE) if name.startswith(f"n={n} ")) for n in WAVE_LENGTHS}
    assert per_length[1] == 14 and per_length[1024] == 14 + 3 * len(RUNS)
