"""Sequence statistics with the counting on the device (td_sequence_stats_device, td_stats.hip) == the host function
(td_sequence_stats_limit), every field of td_seq_stats bit for bit.

get_sequence_stats (src/io.c:52-300) counts bases, read lengths and, for a leading / trailing P segment, the longest exact match of
a linker suffix against the read start / a linker prefix against the read end.  Everything counted is an integer, so the device
sums are exact and the two paths share the finish: nothing here has a tolerance."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

NUC = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
L34 = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC"     # begins with A: the 3' side of the terminator quirk
L34A = "TGGAATTCTCGGGTGCCAAGGAACTCCAGTCACA"    # ends in A: a read one base short of a suffix still matches at the 5' side
assert len(L34) == len(L34A) == 34
ARCHS = {
    "no-p": (["B:ACGT,TTGA", "R:N"], None, None),
    "five-4": (["P:GTCA", "R:N"], "GTCA", None),
    "five-13-n": (["P:TGCANTCGGAAGA", "B:ACGT,TTGA", "R:N"], "TGCANTCGGAAGA", None),
    "three-34": (["R:N", "P:" + L34], None, L34),
    "both-34-4": (["P:" + L34A, "R:N", "P:ACGT"], L34A, "ACGT"),
    "both-13-13": (["P:CCTTGGCACCCGA", "F:NNNN", "R:N", "P:AGATCGGAAGNGC"], "CCTTGGCACCCGA", "AGATCGGAAGNGC"),
}
FIELDS = ["background", "expected_5_len", "expected_3_len", "mean_5_len", "stdev_5_len", "mean_3_len", "stdev_3_len",
          "average_length", "max_seq_len"]


def _codes(s):
    return np.array([NUC[c] for c in s], np.uint8)


def _field_bytes(st, k):
    d = getattr(type(st), k)
    return bytes(st)[d.offset:d.offset + d.size]


def _assert_same(dev, host):
    for k in FIELDS:
        assert _field_bytes(dev, k) == _field_bytes(host, k), (k, getattr(dev, k), getattr(host, k))
    assert bytes(dev) == bytes(host)


def _reads(rng, n, five, three):
    """Ragged reads around the linker lengths mixed with reads of 150: full and truncated linker matches planted, reads one base
    short of a planted 5' suffix, reads that are nothing but a 3' prefix, codes 4 and 5."""
    f = _codes(five) if five else None
    t = _codes(three) if three else None
    L = max(len(five or ""), len(three or ""), 4)
    out = []
    for i in range(n):
        kind = i % 8
        if kind in (0, 2, 6, 7):
            s = rng.integers(0, 4, 150, dtype=np.uint8)
            if kind != 7:
                if f is not None:
                    m = len(f) if kind == 0 else int(rng.integers(4, len(f) + 1))
                    s[:m] = f[len(f) - m:]
                if t is not None:
                    m = len(t) if kind == 0 else int(rng.integers(4, len(t) + 1))
                    s[150 - m:] = t[:m]
        elif kind == 1:
            s = rng.integers(0, 6, int(rng.integers(0, L + 3)), dtype=np.uint8)
        elif kind == 3:
            if f is not None and (i // 8) % 2 == 0:
                m = int(rng.integers(4, len(f) + 1))
                s = f[len(f) - m:len(f) - 1].copy()          # position len reads as the terminator 0 = 'A'
            elif t is not None:
                s = t[:int(rng.integers(3, len(t) + 1))].copy()
            else:
                s = rng.integers(0, 4, int(rng.integers(0, L + 3)), dtype=np.uint8)
        elif kind == 4:
            s = rng.integers(0, 6, 150, dtype=np.uint8)
        else:
            s = rng.integers(0, 4, (i // 8) % 6, dtype=np.uint8)
        out.append(s)
    return out


def _pack(reads, lead=7):
    """codes with `lead` bytes in front that belong to no read, offs[0] = lead."""
    lens = np.array([len(s) for s in reads], np.int64)
    offs = np.zeros(len(reads) + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    offs += lead
    codes = np.concatenate([np.full(lead, 3, np.uint8)] + [np.asarray(s, np.uint8) for s in reads])
    return codes, offs


@pytest.fixture(scope="module")
def ctx():
    from tagdust_amd import TagdustHip
    c = TagdustHip(0)
    c.set_option("specialize", 0)
    yield c
    c.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
@pytest.mark.parametrize("arch", sorted(ARCHS))
def test_device_equals_host(ctx, arch, n):
    from tagdust_amd import lib as tdlib
    segs, five, three = ARCHS[arch]
    rng = np.random.default_rng(n * 31 + len(arch))
    codes, offs = _pack(_reads(rng, n, five, three))
    assert offs[0] != 0
    host = tdlib.sequence_stats(segs, codes, offs)
    dev = tdlib.sequence_stats_device(ctx, segs, codes, offs)
    _assert_same(dev, host)
    if n >= 257:
        assert codes.max() == 5 and int(host.max_seq_len) == 150
        for on, mean, sd in ((five, host.mean_5_len, host.stdev_5_len), (three, host.mean_3_len, host.stdev_3_len)):
            if on and len(on) > 4:   # s0 >= 2 and s0 * s2 != s1^2: the general branch
                assert sd not in (1.0, 10000.0, -1.0) and 4.0 < mean < len(on)
            elif on:                 # a linker of 4 can only match whole
                assert (mean, sd) == (4.0, 10000.0)
            else:
                assert mean == -1.0 and sd == -1.0


def test_one_match_and_equal_matches(ctx):
    """s0 == 1 (mean = expected, stdev 1) and matches of one length only (stdev 10000)."""
    from tagdust_amd import lib as tdlib
    segs, five, three = ARCHS["both-13-13"]
    f, t = _codes(five), _codes(three)
    filler = [np.full(k % 40, 5, np.uint8) for k in range(200)]            # code 5 matches nothing
    one = np.full(60, 5, np.uint8)
    one[:9] = f[4:]
    codes, offs = _pack(filler[:100] + [one] + filler[100:])
    host = tdlib.sequence_stats(segs, codes, offs)
    assert (host.mean_5_len, host.stdev_5_len, host.mean_3_len, host.stdev_3_len) == (13.0, 1.0, 13.0, 1.0)
    _assert_same(tdlib.sequence_stats_device(ctx, segs, codes, offs), host)
    same = []
    for k in range(70):
        s = np.full(50 + k, 5, np.uint8)
        s[:11] = f[2:]
        s[len(s) - 6:] = t[:6]
        same.append(s)
    codes, offs = _pack(filler + same)
    host = tdlib.sequence_stats(segs, codes, offs)
    assert (host.mean_5_len, host.stdev_5_len, host.mean_3_len, host.stdev_3_len) == (11.0, 10000.0, 6.0, 10000.0)
    _assert_same(tdlib.sequence_stats_device(ctx, segs, codes, offs), host)


def test_window(ctx):
    from tagdust_amd import lib as tdlib
    segs, five, three = ARCHS["five-13-n"]
    codes, offs = _pack(_reads(np.random.default_rng(9), 500, five, three))
    host = tdlib.sequence_stats(segs, codes, offs, window=(2, 34))
    assert host.average_length == 32.0
    _assert_same(tdlib.sequence_stats_device(ctx, segs, codes, offs, window=(2, 34)), host)


def test_scan_limit(ctx):
    """1 000 005 reads of 1 to 8 bases: the release flavour's 1 000 001 stops four reads short of the end, the RTEST flavour's
    1 001 000 takes them all; the last reads are the only ones of 8 bases, so the two answers differ."""
    from tagdust_amd import lib as tdlib
    segs = ["P:GTCA", "R:N", "P:ACGT"]     # linkers of 4: reads this short can still match, a read "GTC" through the terminator
    rng = np.random.default_rng(2)
    n = 1000005
    lens = rng.integers(1, 8, n).astype(np.int64)
    lens[-4:] = 8
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    offs += 3
    codes = rng.integers(0, 4, int(offs[-1]), dtype=np.uint8)
    codes[offs[-5]:] = 2
    h_rel = tdlib.sequence_stats(segs, codes, offs, scan_limit=1000001)
    h_all = tdlib.sequence_stats(segs, codes, offs, scan_limit=1001000)
    h_cut = tdlib.sequence_stats(segs, codes[:offs[1000001]], offs[:1000002], scan_limit=1001000)
    assert bytes(h_rel) == bytes(h_cut) and bytes(h_rel) != bytes(h_all)
    assert (h_rel.max_seq_len, h_all.max_seq_len) == (7, 8) and h_rel.stdev_5_len == 10000.0 == h_rel.stdev_3_len
    _assert_same(tdlib.sequence_stats_device(ctx, segs, codes, offs, scan_limit=1000001), h_rel)
    _assert_same(tdlib.sequence_stats_device(ctx, segs, codes, offs, scan_limit=1001000), h_all)


def test_no_reads_is_an_error(ctx):
    from tagdust_amd import TdError
    from tagdust_amd import lib as tdlib
    with pytest.raises(TdError, match="no reads"):
        tdlib.sequence_stats_device(ctx, ["R:N"], np.zeros(1, np.uint8), np.zeros(1, np.int64))
    with pytest.raises(TdError, match="ascending"):
        tdlib.sequence_stats_device(ctx, ["R:N"], np.zeros(8, np.uint8), np.array([0, 5, 3], np.int64))


def test_context_is_left_alone():
    """A context with a model, a resident batch and counters decodes that batch to the same results after a statistics call."""
    from tagdust_amd import TagdustHip
    from tagdust_amd import lib as tdlib
    g = load_golden("c3_b6_s_r_p")
    c = TagdustHip(0)
    try:
        c.set_option("specialize", 0)
        c.upload_model(g)
        c.set_params(float(g["threshold"]), int(g["minlen"]), int(g["dust"]))
        c.upload_batch(g["seq"], g["offs"])
        c.counts_reset()
        c.run()
        before = c.download()
        counts = c.counts()
        segs, five, three = ARCHS["both-13-13"]
        codes, offs = _pack(_reads(np.random.default_rng(4), 3000, five, three))
        _assert_same(tdlib.sequence_stats_device(c, segs, codes, offs), tdlib.sequence_stats(segs, codes, offs))
        assert np.array_equal(c.counts(), counts)
        c.run()
        after = c.download()
        assert np.array_equal(c.counts(), 2 * counts)
    finally:
        c.close()
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(before[0]["read_type"], g["read_type"])
