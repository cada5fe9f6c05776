"""GPU tests (-m gpu) of everything that reads the count table -- list, lookup, profile, read_stats, joint_hist, union, neighbors,
graph_census, list_graph, extend, unitigs, clip (bfcg_kmers.hip, bfcg_lookup.hip, bfcg_readstats.hip, bfcg_tabcmp.hip, bfcg_graph.hip,
bfcg_unitigs.hip, bfcg_clip.hip) -- on the DENSE draws of tests/dense_corpus.py: k = 8..19 with 2 % errors, counted at -b 20 with l_pre
from 4 to 20.  What the constructed fixtures of the other GPU tests never hold is here by itself: several cycles in one call (one of two
nodes), census rows and columns 3 and 4, tips and islands that take three clipping rounds, palindromic k-mers at even k, a table of 16
sub-tables.  For odd k the device is compared WITH THE STRING ORACLES DIRECTLY (tests/test_dense_graph_host.py computes them once) and
with the host twin on the exported table; for even k with the host twin, which that file holds to bfcg_kmer_occ_host.  Every comparison
is exact."""
import functools

import numpy as np
import pytest

import clip_oracle
import dense_corpus
import test_dense_graph_host as H
from dense_corpus import EVEN, ODD, draw
from graph_oracle import census_of_nb, in_mask, paths, planes_of_strs, revcomp, strs_of_planes
from test_kmers_host import decode_slots
from test_lookup_host import stream_kmers

pytestmark = pytest.mark.gpu

U = np.uint64
ALL = ODD + EVEN
# (a): d11 and d19 on region-owned segments that the attach converts, d9 and d13 grown from two slots per sub-table, d15 the host's layout
LAYOUT = {"d9": dict(table_layout=1, tab_cshift=1), "d11": dict(table_layout=0), "d13": dict(table_layout=1, tab_cshift=1), "d15": dict(table_layout=1),
          "d19": dict(table_layout=0), "e8": dict(table_layout=1, tab_cshift=1), "e12": dict(table_layout=0)}


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(gpu_lib, name):
    """a draw counted on the GPU with its l_pre: (a) attached, (c) exported to the host, (b) the export uploaded again -- made once, never
    changed.  The export is the oracle counter's, so every expected value of test_dense_graph_host.py holds for it"""
    c = Case()
    d = draw(name)
    c.k, c.name = d.k, name
    seq, qual, off = d.reads
    c.g = gpu_lib.GpuCounter(d.k, dense_corpus.B, l_pre=d.l_pre, max_batch_pos=len(seq) + len(off) + 64, **LAYOUT[name])
    c.g.count_host(gpu_lib.to_stream(seq, off), gpu_lib.to_stream(qual, off))
    c.g.sync()
    c.segments = bool(c.g.table_info()["segments"])
    c.att = gpu_lib.GpuKmers(c.g)
    c.host = c.g.export_table()
    c.up = gpu_lib.GpuKmers(c.host)
    c.sizes, c.slots = c.host.export_sorted()
    return c


def _sorted(y, *cols):
    """rows (y0, y1, columns...) sorted by the planes"""
    r = np.empty((len(y), 2 + len(cols)), dtype=np.uint64)
    r[:, :2] = y
    for i, col in enumerate(cols):
        r[:, 2 + i] = col
    return r[np.lexsort((r[:, 1], r[:, 0]))]


def _ch(cnt, high):
    return cnt.astype(np.uint16) | high.astype(np.uint16) << 8


def _same_hist(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("name", ALL)
def test_counted_table_is_the_oracles(gpu_lib, name):
    """the export equals the oracle counter's export, as the counting fuzz checks it; d11 and d19 were counted on segments; both device
    forms report the draw's k and l_pre; d15 is a table of 16 sub-tables of 2^7 slots and more"""
    c, d = _case(gpu_lib, name), draw(name)
    sizes, slots, raw = H.counted(name)
    assert np.array_equal(c.sizes, sizes) and np.array_equal(c.slots, slots)
    assert c.segments == (LAYOUT[name].get("table_layout") == 0)
    for km in (c.att, c.up):
        assert (km.k, km.l_pre) == (d.k, d.l_pre) and np.array_equal(km.sub_sizes(), sizes) and _same_hist(km.hist(), c.host.hist())
    if "tab_cshift" in LAYOUT[name]:
        assert c.att.cshift > 1
    if name == "d15":   # a table of 16 sub-tables: the whole-wave branch of the sizes passes, long probe chains
        assert len(c.att.sub_sizes()) == 16 and c.att.cshift >= 7 and c.up.cshift >= 7 and sizes.min() > 64


@pytest.mark.parametrize("name", ALL)
def test_neighbors_census_and_listing(gpu_lib, name):
    """on (a) and (b), at min_cnt 1 and 2: the eight neighbours of every node, of reverse complements and of absent k-mers; the census;
    list_graph under five masks -- against the string oracle (odd k; bfcg_kmer_occ_host one by one for even k) and against the host twin.
    The census of the draws with k <= 13 has nodes in rows or columns 3 and 4 ON THE DEVICE; the even tables list at least five k-mers
    that are their own reverse complement, and these are among the queries"""
    c = _case(gpu_lib, name)
    y, strs, ch = H.nodes(gpu_lib, name)
    q, want = H.nb_queries(gpu_lib, name)[1], H.want_neighbors(gpu_lib, name)
    assert np.array_equal(c.host.neighbors(q), want)
    for km in (c.att, c.up):
        assert np.array_equal(km.neighbors(q), want)
    for min_cnt in (1, 2):
        nb, node = H.want_nb(gpu_lib, name, min_cnt), (ch & 0xff) >= min_cnt
        deg = census_of_nb(nb[node])
        assert np.array_equal(c.host.graph_census(min_cnt), deg)
        for km in (c.att, c.up):
            got = km.graph_census(min_cnt)
            assert np.array_equal(got, deg)
            if min_cnt == 1 and c.k % 2 and c.k <= 13:   # census rows or columns 3 and 4
                assert got[4, :].sum() + got[:, 4].sum() >= 1 and got.sum() - got[:3, :3].sum() >= 5
            for m in H.MASKS:
                mask = gpu_lib.GRAPH_MASKS[m]
                keep = node & in_mask(nb, mask)
                ly, lc, lh, lnb = km.list_graph(min_cnt, mask)
                assert np.array_equal(_sorted(ly, _ch(lc, lh), lnb), _sorted(y[keep], ch[keep], nb[keep])), (min_cnt, m)
                ty, tc, th, tnb = c.host.list_graph(min_cnt, mask)
                assert np.array_equal(_sorted(ly, _ch(lc, lh), lnb), _sorted(ty, _ch(tc, th), tnb)), (min_cnt, m)
    if c.k % 2 == 0:   # palindromic k-mers at even k
        listed = strs_of_planes(c.att.list()[0], c.k)
        pal = [s for s in listed if s == revcomp(s)]
        assert len(pal) >= 5
        py = planes_of_strs(pal, c.k)
        assert np.array_equal(c.att.neighbors(py), c.host.neighbors(py)) and np.array_equal(c.up.lookup(py), c.host.occ_planes(py)) and (c.up.lookup(py) >= 0).all()


@pytest.mark.parametrize("name", ALL)
def test_extend(gpu_lib, name):
    """300 nodes and 20 absent k-mers from both strands, max_len 1, 7 and 300, min_cnt 1 and 2: paths, lengths and stop codes are the
    string oracle's and the host twin's; max_len 0 is refused as the twin refuses it"""
    c = _case(gpu_lib, name)
    strs, y = H.seeds(gpu_lib, name)
    for min_cnt in (1, 2):
        for max_len in H.MAX_LENS:
            want = H.want_extend(gpu_lib, name, min_cnt, max_len)
            twin = c.host.extend(y, min_cnt, max_len)
            assert paths(twin[0], twin[1]) == [w[0] for w in want] and list(twin[2]) == [w[1] for w in want]
            for km in (c.att, c.up):
                got = km.extend(y, min_cnt, max_len)
                assert paths(got[0], got[1]) == [w[0] for w in want] and list(got[2]) == [w[1] for w in want], (min_cnt, max_len)
                assert all(np.array_equal(a, b) for a, b in zip(got, twin))
    with pytest.raises(gpu_lib.BfcGpuError, match=r"max_len 0 is outside \[1, 65535\]"):
        c.att.extend(y, 1, 0)


@pytest.mark.parametrize("name", ODD)
def test_unitigs(gpu_lib, name):
    """on (a) and (b), at min_cnt 1 and 2: the sorted unitigs are the string oracle's and the host twin's.  SEVERAL CYCLES IN ONE CALL,
    AMONG THEM THE TWO-NODE CYCLE, come back from the device: at least four for k >= 11, the cycle of AC in every draw"""
    c = _case(gpu_lib, name)
    for min_cnt in (1, 2):
        want = H.want_unitigs(gpu_lib, name, min_cnt)
        assert gpu_lib.unitig_rows(*c.host.unitigs(min_cnt)) == want
        for km in (c.att, c.up):
            seq, off, nk, cs, ends = km.unitigs(min_cnt)
            assert off[0] == 0 and off[-1] == len(seq) and np.array_equal(np.diff(off).astype(np.int64), nk.astype(np.int64) + c.k - 1)
            got = gpu_lib.unitig_rows(seq, off, nk, cs, ends)
            assert got == want
            cyc = [r for r in got if r[5]]
            two = [r for r in cyc if r[1] == 2]
            assert len(cyc) >= (4 if c.k >= 11 else 2) and len(two) == 1 and two[0][0] == (b"AC" * c.k)[:c.k + 1]
            assert int(nk.sum()) == int(km.graph_census(min_cnt).sum())


def _listing(km):
    """{canonical string: high << 8 | count} of a device table (odd k)"""
    y, cnt, high = km.list()
    return {min(s, revcomp(s)): int(v) for s, v in zip(strs_of_planes(y, km.k), _ch(cnt, high))}


@pytest.mark.parametrize("i", [0, 1, 2])
@pytest.mark.parametrize("name", ODD)
def test_clip(gpu_lib, name, i):
    """on (a) and (b), for each of the three parameter sets: the result's listing, the stats and the result's unitigs(1) are the string
    oracle's and the host twin's; the input's hist() is unchanged; the result chains -- graph_census, clip again with islands, to_host --
    and the exported table is the oracle clipped twice.  THREE CLIPPING ROUNDS run on the device for d9 and d11 with the first set"""
    c = _case(gpu_lib, name)
    kw = H.clip_sets(c.k)[i]
    surv, stats, units = H.want_clip(gpu_lib, name, i)
    surv2 = H.want_clip(gpu_lib, name, i, True)[0]
    tw, tw_stats = c.host.clip(**kw)
    assert clip_oracle.survivors_of_table(tw) == surv and H.stats_of(tw_stats) == stats
    tw.close()
    for km in (c.att, c.up):
        before = km.hist()
        res, got = km.clip(**kw)
        assert H.stats_of(got) == stats and _listing(res) == surv
        if i == 0 and name in ("d9", "d11"):   # clipping of at least three rounds
            assert len(got) >= 3
        assert gpu_lib.unitig_rows(*res.unitigs(1)) == units
        assert _same_hist(km.hist(), before)
        assert int(res.graph_census(1).sum()) == len(surv)
        again, _ = res.clip(**dict(kw, islands=True))
        host = again.to_host()
        assert clip_oracle.survivors_of_table(host) == surv2 and host.count() == len(surv2)
        for o in (host, again, res):
            o.close()


@pytest.mark.parametrize("name", ALL)
def test_union_with_itself_and_joint_hist(gpu_lib, name):
    """a.union(a) holds the same k-mers with count and high count doubled (saturating at 63 for the high count; no count of a draw
    reaches 128), so for odd k the same unitigs with doubled cnt_sum; joint_hist(a, a) is diagonal and its diagonal is hist()"""
    c = _case(gpu_lib, name)
    assert int((c.slots & U(0xff)).max()) < 128
    for km in (c.att, c.up):
        u = km.union(km)
        y, cnt, high = km.list()
        uy, ucnt, uhigh = u.list()
        assert np.array_equal(_sorted(uy, ucnt, uhigh), _sorted(y, 2 * cnt.astype(np.uint64), np.minimum(2 * high.astype(np.uint64), U(63))))
        if c.k % 2:
            want = H.want_unitigs(gpu_lib, name, 1)
            got = gpu_lib.unitig_rows(*u.unitigs(1))
            assert [r[:2] + r[3:] for r in got] == [r[:2] + r[3:] for r in want] and [r[2] for r in got] == [2 * r[2] for r in want]
        u.close()
        joint, shared, only_a, only_b = km.joint_hist(km)
        assert (shared, only_a, only_b) == (len(c.slots), 0, 0)
        assert np.array_equal(np.diag(joint), km.hist()[1]) and int(joint.sum()) == shared


@pytest.mark.parametrize("name", ALL)
def test_list_and_lookup(gpu_lib, name):
    """list() -- all sub-tables, then three sub_lo / sub_hi pieces -- equals the host decode of the export's slots; lookup() of every
    node on either strand and of 500 absent k-mers equals the dict (odd k) and bfcg_kmers_occ_host"""
    c, d = _case(gpu_lib, name), draw(name)
    hy, hch = decode_slots(gpu_lib._lib.load(), c.k, d.l_pre, c.sizes, c.slots)
    want = _sorted(hy, hch)
    y, strs, ch = H.nodes(gpu_lib, name)
    q = strs + [revcomp(s) for s in strs[::3]] + H.absent(gpu_lib, name, 500)
    qy = planes_of_strs(q, c.k)
    occ = c.host.occ_planes(qy)
    if c.k % 2:
        g = H.graph(gpu_lib, name)
        assert np.array_equal(occ, np.array([g.value(s) for s in q], dtype=np.int16))
    assert (occ[:len(strs)] >= 0).all() and (occ[-500:] == -1).all()
    n_sub = len(c.sizes)
    cuts = [0, n_sub // 3 + 1, n_sub - 1, n_sub]
    for km in (c.att, c.up):
        ly, lc, lh = km.list()
        assert np.array_equal(_sorted(ly, _ch(lc, lh)), want)
        parts = [km.list(sub_lo=lo, sub_hi=hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
        assert [len(p[1]) for p in parts] == [int(c.sizes[lo:hi].sum()) for lo, hi in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(_sorted(*[np.concatenate([p[j] for p in parts]) for j in range(3)]), _sorted(ly, lc, lh))
        assert np.array_equal(km.lookup(qy), occ) and km.n_found == int((occ >= 0).sum())


@pytest.mark.parametrize("name", ALL)
def test_profile_and_read_stats(gpu_lib, name):
    """the draw's first 300 reads: profile() is bfcg_kmers_occ_host of the k-mer ending at every position, read_stats() at min_cov 1 and
    3 is HostTable.read_stats"""
    c = _case(gpu_lib, name)
    seq, qual, off = draw(name).reads
    n = 300
    stream = gpu_lib.to_stream(seq[:int(off[n])], off[:n + 1])
    soff = off[:n + 1] + np.arange(n + 1, dtype=np.uint64)
    ends, y = stream_kmers(stream, c.k)
    prof = np.where(ends, c.host.occ_planes(y), -2).astype(np.int16)
    assert (prof >= 0).any() and (prof == -1).any() and (prof == -2).any()
    stats = {mc: c.host.read_stats(stream, soff, mc) for mc in (1, 3)}
    assert (stats[3][:, 2] > 0).any() and (stats[1][:, 2] > stats[3][:, 2]).any()
    for km in (c.att, c.up):
        assert np.array_equal(km.profile(stream), prof)
        for mc in (1, 3):
            assert np.array_equal(km.read_stats(stream, soff, mc), stats[mc])


@pytest.mark.parametrize("name", EVEN)
def test_even_k_refuses_unitigs_and_clip(gpu_lib, name):
    """unitigs and clip are refused for even k with the existing message, and the object still answers"""
    c = _case(gpu_lib, name)
    for km in (c.att, c.up):
        for call in (km.unitigs, km.clip):
            with pytest.raises(gpu_lib.BfcGpuError, match="k=%d is even" % c.k):
                call()
        assert _same_hist(km.hist(), c.host.hist())


# ---- seams, on d11 ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [1, 64])
def test_launch_cap(gpu_lib, monkeypatch, cap):
    """BFCG_UNITIG_CAP (read when the object is made) of 1 and 64: the draw's cycles put more than 64 candidates into the cycles' walk,
    its dead ends cut the clipping walks into many launches; unitigs and clip give the rows of the default"""
    c = _case(gpu_lib, "d11")
    monkeypatch.setenv("BFCG_UNITIG_CAP", str(cap))
    small = gpu_lib.GpuKmers(c.g)
    monkeypatch.delenv("BFCG_UNITIG_CAP")
    for min_cnt in (1, 2):
        want = H.want_unitigs(gpu_lib, "d11", min_cnt)
        assert sum(r[1] for r in want if r[5]) > 64 and sum(1 for r in want if not r[5]) > 64
        assert gpu_lib.unitig_rows(*small.unitigs(min_cnt)) == want
    for i in (0, 1):
        surv, stats, units = H.want_clip(gpu_lib, "d11", i)
        res, got = small.clip(**H.clip_sets(c.k)[i])
        assert H.stats_of(got) == stats and sum(s[0] for s in stats) > (64 if i == 0 else 1) and _listing(res) == surv
        assert gpu_lib.unitig_rows(*res.unitigs(1)) == units
        res.close()
    small.close()


def test_candidate_buffer_grows_between_calls(gpu_lib):
    """on one fresh object unitigs(2), unitigs(1), unitigs(2): the buffer of the cycles' candidates is sized by the first call, has to
    grow for the second (the low-count circle adds 33 nodes) and is larger than needed for the third; all three are the oracle's"""
    c = _case(gpu_lib, "d11")
    one, two = H.want_unitigs(gpu_lib, "d11", 1), H.want_unitigs(gpu_lib, "d11", 2)
    assert sum(r[1] for r in one if r[5]) == sum(r[1] for r in two if r[5]) + dense_corpus.LOW_CIRC
    fresh = gpu_lib.GpuKmers(c.g)
    for min_cnt, want in ((2, two), (1, one), (2, two)):
        assert gpu_lib.unitig_rows(*fresh.unitigs(min_cnt)) == want
    fresh.close()
