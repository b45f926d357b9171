"""Helpers of tests/test_gpu_table_layout.py: keys placed by chosen hash, and a reference that owes nothing to the table.

A table slot is addressed by the TOP s bits of a key's mixed hash (csrc/kmer.hpp: home_of), so a test that chooses hashes chooses
home slots: `craft` draws hashes with a given home (and, if asked, a given remainder), turns them back into k-mers through the
library's inverse mix (jasper_debug_mix) and keeps those that are their own canonical form -- such a key can be imported as a raw
hash, counted as bases and looked up as a string alike.  The reference is a Python Counter keyed by canonical k-mer STRING with
Python ints as counts; canonical form is decided on strings (reverse complement, string minimum), never by the code under test.
"""
import collections
import ctypes as C
import re

M64 = (1 << 64) - 1
U32 = (1 << 32) - 1
MAXPROBE = 1024          # csrc/kmer.hpp: probe offsets 0..1023 live in the tag's low 10 bits
TAG_REM_BITS = 53        # ... which leaves 53 remainder bits in the tag word
HISTO_BINS = 10002
_C1 = 0x9E3779B97F4A7C15
_COMP = str.maketrans("ACGT", "TGCA")
_COMPB = bytes.maketrans(b"ACGT", b"TGCA")


# ---- the hash, restated (csrc/kmer.hpp: mix) -- the inverse is NOT restated: decode() goes through the library ------------------
def py_mix(x, B):
    """mixed hash of the B-bit key x (B = 2k)"""
    if B <= 64:
        m, h = (1 << B) - 1, B // 2
        v = x & m
        v ^= v >> h
        v = (v * _C1) & m
        v ^= v >> h
        return v
    hb = B - 64
    lo = x & M64
    lo ^= lo >> 32
    lo = (lo * _C1) & M64
    lo ^= lo >> 29
    rot = ((lo >> 30) | (lo << 34)) & M64
    return ((((x >> 64) ^ rot) & ((1 << hb) - 1)) << 64) | lo


# ---- k-mers as strings -----------------------------------------------------------------------------------------------
_FOUR = ["".join("ACGT"[(b >> sh) & 3] for sh in (6, 4, 2, 0)) for b in range(256)]


def kmer_of_int(x, k):
    """the first base is the most significant bit pair"""
    assert 0 <= x < (1 << (2 * k)) and 1 <= k <= 64
    return "".join([_FOUR[b] for b in x.to_bytes(16, "big")])[64 - k:]


def int_of_kmer(s):
    x = 0
    for ch in s:
        x = (x << 2) | "ACGT".index(ch)
    return x


def revcomp(s):
    return s.translate(_COMP)[::-1]


def canon(s):
    r = revcomp(s)
    return s if s <= r else r


def _lib():
    from jasper_amd import _lib as L
    return L.lib()


def unmix_lib(k, h):
    out = (C.c_uint64 * 2)()
    assert _lib().jasper_debug_mix(k, 1, h >> 64, h & M64, out) == 0
    return (out[0] << 64) | out[1]


def decode(k, h):
    """the k-mer whose mixed hash is h"""
    return kmer_of_int(unmix_lib(k, h), k)


def hash_of_kmer(s):
    """mixed hash of the canonical form of s, through the Python restatement (for keys that are chosen as strings)"""
    return py_mix(int_of_kmer(canon(s)), 2 * len(s))


# ---- geometry (csrc/kmer.hpp) ---------------------------------------------------------------------------------------
def is_wide(k, s):
    """a table of 2^s slots keeps the low 64 remainder bits of a key in a second word per slot"""
    return 2 * k - s > TAG_REM_BITS


def split(k, s, h):
    """(home, tag remainder, ext word or None) of hash h in a table of 2^s slots"""
    rb = 2 * k - s
    rem = h & ((1 << rb) - 1)
    if is_wide(k, s):
        return h >> rb, rem >> 64, rem & M64
    return h >> rb, rem, None


def join(k, s, home, tag_rem, ext=None):
    rb = 2 * k - s
    rem = tag_rem if ext is None else (tag_rem << 64) | ext
    assert 0 <= home < (1 << s) and 0 <= rem < (1 << rb)
    return (home << rb) | rem


def part_of(k, h, nparts):
    """owner partition of a key: floor(top32(hash) * nparts / 2^32)"""
    B = 2 * k
    top32 = h >> (B - 32) if B >= 32 else h << (32 - B)
    return (top32 * nparts) >> 32


def last_home_of_part(s, part, nparts):
    """the last home slot (s <= 32) whose first hash belongs to partition `part`"""
    sh = 32 - s
    home = min((((part + 1) << 32) // nparts) >> sh, (1 << s) - 1)
    while ((home << sh) * nparts) >> 32 > part:
        home -= 1
    assert ((home << sh) * nparts) >> 32 == part
    return home


def log2_slots(t):
    n = t.info()["slots"]
    assert n & (n - 1) == 0
    return n.bit_length() - 1


# ---- crafting --------------------------------------------------------------------------------------------------------
def craft(k, s, home, n, rng, canonical=True, rem=None):
    """n distinct hashes (Python ints) whose top s bits are `home`, and their k-mer strings.

    rem: None = random remainders; a callable rng -> remainder; or an iterable of remainders tried in order (n = None then takes
    every one that passes).  canonical: keep only hashes whose k-mer is <= its reverse complement.  About half of all hashes
    pass, so at most 8 n candidates are looked at."""
    B = 2 * k
    rb = B - s
    assert 0 <= s <= B and 0 <= home < (1 << s)
    if rem is None:
        draw = (rng.getrandbits(rb) if rb else 0 for _ in iter(int, 1))
    elif callable(rem):
        draw = (rem(rng) for _ in iter(int, 1))
    else:
        draw = iter(rem)
    hashes, kmers, seen, tried = [], [], set(), 0
    for r in draw:
        if n is not None and len(hashes) >= n:
            break
        tried += 1
        assert n is None or tried <= 8 * n, "craft: more than 8 n candidates"
        assert 0 <= r < (1 << rb)
        h = (home << rb) | r
        if h in seen:
            continue
        seen.add(h)
        km = decode(k, h)
        if canonical and km > revcomp(km):
            continue
        hashes.append(h)
        kmers.append(km)
    assert n is None or len(hashes) == n, "craft: the remainders given do not yield n keys"
    return hashes, kmers


def craft_edge(k, s, first_home, n_homes, n_keys, rng):
    """n_keys keys spread evenly over the homes first_home .. first_home + n_homes - 1 (mod 2^s); the cap of 8 candidates per key
    holds for the whole set (a single key of a single home misses it once in 256 times)"""
    rb = 2 * k - s
    hs, ks, tried = [], [], 0
    for i in range(n_homes):
        home = (first_home + i) & ((1 << s) - 1)
        m = n_keys // n_homes + (1 if i < n_keys % n_homes else 0)
        mine = set()
        while len(mine) < m:
            tried += 1
            assert tried <= 8 * n_keys, "craft_edge: more than 8 n candidates"
            h = (home << rb) | rng.getrandbits(rb)
            km = decode(k, h)
            if h in mine or km > revcomp(km):
                continue
            mine.add(h)
            hs.append(h)
            ks.append(km)
    return hs, ks


def entries(hashes, counts):
    """numpy [n, 3] array for KmerTable.import_entries: hash.hi, hash.lo, count"""
    import numpy as np
    return np.array([[h >> 64, h & M64, c] for h, c in zip(hashes, counts)], dtype=np.uint64).reshape(-1, 3)


def pack(k, h, c):
    """16-byte exchange entry { hash.lo, hash.hi | count << (2k - 64) } (2k <= 64: { hash, count })"""
    B = 2 * k
    if B <= 64:
        assert c <= M64
        return h, c
    assert c < (1 << (128 - B))
    return h & M64, (h >> 64) | (c << (B - 64))


def unpack(k, w0, w1):
    B = 2 * k
    if B <= 64:
        return w0, w1
    return ((w1 & ((1 << (B - 64)) - 1)) << 64) | w0, w1 >> (B - 64)


def packed_tensor(k, pairs, device):
    """a [n, 2] int64 device tensor of packed entries from (hash, count) pairs"""
    import numpy as np
    import torch
    a = np.array([pack(k, h, c) for h, c in pairs], dtype=np.uint64).reshape(-1, 2)
    return torch.from_numpy(a.view(np.int64)).to(device)


def unpacked(k, tensor, n):
    """[(hash, count)] of the first n entries of such a tensor"""
    import numpy as np
    a = tensor[:n].cpu().numpy().view(np.uint64)
    return [unpack(k, int(w0), int(w1)) for w0, w1 in a]


# ---- the reference -----------------------------------------------------------------------------------------------------
def kmer_counter(text, k):
    """canonical k-mer string -> occurrences in a base stream (bytes or str): every maximal stretch of >= k ACGT bytes walked"""
    b = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    d = collections.Counter()
    for m in re.finditer(rb"[ACGT]{%d,}" % k, b.upper()):
        t = m.group()
        for i in range(len(t) - k + 1):
            km = t[i:i + k]
            rc = km.translate(_COMPB)[::-1]
            d[(km if km <= rc else rc).decode()] += 1
    return d


class Ref:
    """what a table must hold: canonical k-mer string -> count (Python ints, never clamped)"""

    def __init__(self, k):
        self.k = k
        self.c = collections.Counter()
        self.occurrences = 0          # k-mer occurrences added by COUNTING (what info()["occurrences"] reports; imports add none)

    def copy(self):
        r = Ref(self.k)
        r.c = collections.Counter(self.c)
        r.occurrences = self.occurrences
        return r

    def add_kmers(self, kmers, counts):
        for km, c in zip(kmers, counts):
            assert len(km) == self.k and km == canon(km), "the reference is keyed by canonical strings"
            if c:
                self.c[km] += c
        return self

    def add_hashes(self, hashes, counts):
        return self.add_kmers([decode(self.k, h) for h in hashes], counts)

    def add_counter(self, counter, times=1):
        for km, c in counter.items():
            self.c[km] += c * times
        self.occurrences += sum(counter.values()) * times
        return self

    def add_bases(self, text, times=1):
        return self.add_counter(kmer_counter(text, self.k), times)

    def clamped(self):
        r = Ref(self.k)
        r.c = collections.Counter({km: min(c, U32) for km, c in self.c.items()})
        return r

    def filtered(self, pred):
        """the keys whose mixed hash satisfies pred (hashes through the Python restatement of mix)"""
        r = Ref(self.k)
        r.c = collections.Counter({km: c for km, c in self.c.items() if pred(py_mix(int_of_kmer(km), 2 * self.k))})
        return r

    @property
    def distinct(self):
        return len(self.c)

    def histogram(self):
        h = [0] * HISTO_BINS
        for c in self.c.values():
            h[min(min(c, U32), 10001)] += 1
        return h

    def lookup(self, strings):
        return [min(self.c.get(canon(s.upper()), 0), U32) for s in strings]

    def spectrum(self, asm):
        """cells[m][c] of KmerTable.spectrum: m = min(copies in asm, 5), c = min(min(count here, 2^32-1), 10001); column 0 = only in asm"""
        S = [[0] * HISTO_BINS for _ in range(6)]
        for km, c in self.c.items():
            S[min(asm.c.get(km, 0), 5)][min(min(c, U32), 10001)] += 1
        for km, m in asm.c.items():
            if km not in self.c:
                S[min(m, 5)][0] += 1
        return S

    def report(self, seqs, thre):
        """(counts, runs) of KmerTable.kmer_report: per sequence (windows, valid, unreliable, absent); runs of consecutive unreliable
        windows (seq, start, n_kmers, n_absent, min_count); unreliable = valid and clamped count < thre"""
        k, counts, runs = self.k, [], []
        for si, s in enumerate(seqs):
            valid = unrel = absent = 0
            cur = None
            nwin = max(0, len(s) - k + 1)
            for i in range(nwin):
                w = s[i:i + k].upper()
                c = min(self.c.get(canon(w), 0), U32) if re.fullmatch("[ACGT]*", w) else None
                if c is not None:
                    valid += 1
                    absent += c == 0
                if c is not None and c < thre:
                    unrel += 1
                    if cur is None:
                        cur = [si, i, 0, 0, c]
                    cur[2] += 1
                    cur[3] += c == 0
                    cur[4] = min(cur[4], c)
                elif cur is not None:
                    runs.append(tuple(cur))
                    cur = None
            if cur is not None:
                runs.append(tuple(cur))
            counts.append((nwin, valid, unrel, absent))
        return counts, runs


def table_dict(t):
    """export_entries() decoded to {k-mer string: count}; every key once"""
    e = t.export_entries()
    d = {}
    for hi, lo, c in e.tolist():
        d[decode(t.k, (hi << 64) | lo)] = c
    assert len(d) == len(e), "export_entries: a key appears twice"
    return d


def _diff(got, want, limit=6):
    bad = [(km, got.get(km), want.get(km)) for km in set(got) | set(want) if got.get(km) != want.get(km)]
    return "%d keys differ (k-mer, table, reference): %s" % (len(bad), sorted(bad)[:limit])


def check_table(t, ref, absent=(), present=None, occurrences=None):
    """every comparison of a table with the reference, bit-exact: the exported entries, info()["distinct"], the histogram and
    lookup() of the reference's keys (or of `present`, a sample of them) and of `absent` (keys that must read 0)"""
    want = dict(ref.c)
    got = table_dict(t)
    assert got == want, _diff(got, want)
    info = t.info()
    assert info["distinct"] == ref.distinct
    if occurrences is not None:
        assert info["occurrences"] == occurrences
    assert t.histogram() == ref.histogram()
    keys = list(want) if present is None else list(present)
    assert t.lookup(keys) == ref.lookup(keys)
    assert t.lookup([revcomp(km) for km in keys[:256]]) == ref.lookup(keys[:256])
    absent = list(absent)
    if absent:
        assert all(canon(km) not in ref.c for km in absent)
        assert t.lookup(absent) == [0] * len(absent)


def absent_neighbours(k, s, hashes, taken, rng, per_key=2):
    """canonical k-mers that are NOT in `taken` (a container of k-mer strings) but share, with one of `hashes` in a table of 2^s
    slots: the home; in a wide table also home + tag remainder (another ext word) and home + ext word (another tag remainder)"""
    out = []
    rb = 2 * k - s

    def some(rems):          # the canonical ones among a few candidates (no quota: a single key misses the cap of 8 once in 256 times)
        return craft(k, s, home, None, rng, rem=rems)[1][:per_key]

    for h in hashes:
        home, tag_rem, ext = split(k, s, h)
        out += some([rng.getrandbits(rb) for _ in range(4 * per_key)])
        if ext is not None:
            eb = min(64, rb)                      # bits of the ext word in use
            out += some([(tag_rem << 64) | rng.getrandbits(eb) for _ in range(4 * per_key)])
            flips = [1 << b for b in (0, 1, 2, 3, 4, 31, 32, eb - 1)]          # one bit away, in either 32-bit half
            out += craft(k, s, home, None, rng, rem=[(tag_rem << 64) | (ext ^ f) for f in flips])[1]
            if rb > 64:
                out += some([(rng.getrandbits(rb - 64) << 64) | ext for _ in range(4 * per_key)])
                out += craft(k, s, home, None, rng, rem=[((tag_rem ^ (1 << b)) << 64) | ext for b in range(min(4, rb - 64))])[1]
    return [km for km in dict.fromkeys(out) if km not in taken]


def region_edge_keys(k, s, rbits, rng, per_cluster=64, edge=16, blockers=32, chain=600):
    """the crafted keys of the counting scenario for a table of 2^s slots counted in regions of 2^rbits slots: name -> (hashes,
    k-mers).  "edge": per_cluster keys homed in the last `edge` slots of a region; "last": the same for the table's last region;
    "blocked": the same for a region whose successor's first `blockers` home slots each hold one of "blockers"; "chain": `chain`
    keys on one home, chain/2 slots before a region's end."""
    R, nreg = 1 << rbits, 1 << (s - rbits)
    assert nreg >= 8 and per_cluster > edge and chain // 2 < R and chain < MAXPROBE
    r_edge, r_blocked, r_chain = nreg // 5, nreg // 2, nreg // 3
    return {
        "edge": craft_edge(k, s, (r_edge + 1) * R - edge, edge, per_cluster, rng),
        "last": craft_edge(k, s, nreg * R - edge, edge, per_cluster, rng),
        "blocked": craft_edge(k, s, (r_blocked + 1) * R - edge, edge, per_cluster, rng),
        "blockers": craft_edge(k, s, (r_blocked + 1) * R, blockers, blockers, rng),
        "chain": craft(k, s, (r_chain + 1) * R - chain // 2, chain, rng),
    }
