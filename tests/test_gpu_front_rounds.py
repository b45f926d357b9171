"""GPU: the sixteen-per-round seam of the extend step that the four front searches share (front_extend in csrc/front_search.hpp): the mixed
insertions and the het clusters of the indel scan, the compound scan and the gap search, each on one site or candidate whose frontier is
exactly 16, 17, 32, 33, 48 and 49 strings wide -- one, two, three and four rounds, full ones and ones with a single parent.  (64 and 65
are the cap tests of the four searches' own files.)  Expected records, counters and statuses are those of the restatements in the four
*_host.py files, fed by Python dicts of canonical k-mer strings; nothing expected here comes from the code under test.

The workload, at k = 21 and thre 1: left and right are 150 random bases each, c is a base that right does not start with, and the reads
are left + right with c + (a string of six bases) planted between the two, w strings that differ pairwise in their first three bases.
Whatever is searched from the 20 bases before c holds 1, up to 4, up to 16 and then w strings, and keeps w of them while the strings
run on into `right`.
  mixed, clusters   the contig is left + right and is a read too: the candidate is (len(left), c).  (c comes first because a candidate's
                    strings all start with its base: six-base strings that differ in their first three bases cannot all do so.)  A pure
                    insertion is no het cluster, so for the clusters the reads also hold c2 in place of the first base of right.
  compound          the contig holds c2 c2 c2 between left and right, c2 another base than c that no string ends with (a string that
                    ended as the contig's own bytes do would shorten the site), and is no read: one site.
  gaps              the contig is left + c + right, searched at the explicit site behind c (a = q).  From 17 strings on the level at
                    which they all end is more than the site may list, so the site is complex there: its levels and status are checked,
                    and the records at w = 16."""
import numpy as np
import pytest

from test_compound_host import FRONT, restate_compound
from test_gaps_host import restate_gap_search
from test_gpu_compound import check as check_compound
from test_gpu_copies import dict_counter, kmer_dict
from test_gpu_gaps import check_result as check_gaps
from test_gpu_het_clusters import check as check_clusters
from test_gpu_indels_mixed import check as check_mixed
from test_het_clusters_host import restate_clusters
from test_indels_host import ACGT, rand_bases
from test_indels_mixed_host import plant_strings, restate_mixed

pytestmark = pytest.mark.gpu

K, LEN = 21, 8                      # LEN: max_len and cluster_len, one more than the planted c + six bases
WIDTHS = (16, 17, 32, 33, 48, 49)
SEARCHES = ("mixed", "clusters", "compound", "gaps")


def front_workload(search, w):
    """(reads, contig, at): at = len(left), where the strings are planted"""
    rng = np.random.default_rng(4000 + w)
    left, right = rand_bases(rng, 150), rand_bases(rng, 150)
    c, c2 = [bytes([b]) for b in ACGT if b != right[0]][:2]
    firsts = [bytes(ACGT[(v >> s) & 3] for s in (4, 2, 0)) for v in rng.permutation(64)[:w]]
    lasts = [bytes([b]) for b in ACGT if bytes([b]) != c2]
    strings = [f + rand_bases(rng, 2) + lasts[int(rng.integers(0, 3))] for f in firsts]
    assert len({y[:3] for y in strings}) == w and all(len(y) == 6 for y in strings)
    at = len(left)
    planted = [plant_strings(left + right, [(at, "ins", c + y)]) for y in strings]
    if search == "mixed":
        return [left + right] + planted, left + right, at
    if search == "clusters":
        return [left + right] + [plant_strings(left + right, [(at, "ins", c + y + c2), (at, "del", 1)]) for y in strings], left + right, at
    if search == "compound":
        return planted, plant_strings(left + right, [(at, "ins", c2 * 3)]), at
    return planted, plant_strings(left + right, [(at, "ins", c)]), at


def expected(search, w):
    """(reads, contig, at, the restatement's result, the level sizes it computed as one flat list)"""
    reads, contig, at = front_workload(search, w)
    count = dict_counter(kmer_dict(reads, K))
    st = {}
    if search == "mixed":
        want = restate_mixed([contig], K, count, 1, LEN, st)
    elif search == "clusters":
        want = restate_clusters([contig], K, count, 1, LEN, st)
    elif search == "compound":
        want = restate_compound([contig], K, count, 1, LEN, st)
    else:
        want = restate_gap_search([contig], K, count, 1, LEN, [(0, at + 1, at + 1, 0)], st)
        st["levels"] = [n for lv in st["levels"] for n in lv]
    return reads, contig, at, want, st["levels"]


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable, _lib
    assert _lib.lib().jasper_indel_front() == FRONT and KmerTable.compound_front() == FRONT and KmerTable.gap_front() == FRONT
    return KmerTable


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("search", SEARCHES)
def test_a_front_of_w_strings(KT, search, w):
    reads, contig, at, want, levels = expected(search, w)
    assert w in levels and max(levels) <= FRONT, (search, w, levels)       # the construction, before the GPU is touched
    if search == "gaps":                                                    # (status, records, levels) of the site
        assert want[1][0][4:7] == (("limit", w, LEN) if w <= 16 else ("complex", 0, 6)), want[1]
    else:
        assert len(want[1]) == w, (search, w, len(want[1]))                 # every string is a record
    t = KT(K, min_slots=1 << 16)
    t.count_bases(b"N".join(reads))
    if search == "mixed":
        check_mixed(t, [contig], 1, LEN, want, (search, w))
    elif search == "clusters":
        check_clusters(t, [contig], 1, LEN, want, (search, w))
    elif search == "compound":
        check_compound(t, [contig], 1, LEN, want, (search, w))
    else:
        check_gaps(t.gap_search([contig], 1, LEN, [(0, at + 1, at + 1, 0)]), want, (search, w))
    t.close()
