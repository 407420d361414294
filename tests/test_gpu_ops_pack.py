"""GPU tests of pack_kernel (cmpc_pack_weights / cmpc_pack_weights_range) on synthetic descriptor tables, byte for byte against the
restatement in tests/packref.py.  The arena starts as a sentinel NaN pattern: every byte a descriptor covers (padding included) must
equal the restatement, every other byte must keep the sentinel."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from tests import packref as PR

L = importlib.import_module("cmpc-refseg_amd._lib")
SENTINEL = np.array([0xA5, 0xA5, 0xA5, 0x7F], dtype=np.uint8)      # float32 0x7FA5A5A5: a signalling NaN


def desc(dt, tr, Kp, Np, ks, ns, src_off, ld_src, ld_pad=0):
    d = L.PackDesc()
    d.src_off, d.ld_src, d.dst_dt, d.transpose = src_off, ld_src, dt, tr
    d.rows, d.cols = (Np, Kp) if tr else (Kp, Np)
    d.ld_dst = d.cols + ld_pad
    d.nks = len(ks)
    for i, (s, l, t) in enumerate(ks):
        d.ks_src[i], d.ks_len[i], d.ks_dst[i] = s, l, t
    d.nns = len(ns)
    for i, (s, l, t) in enumerate(ns):
        d.ns_src[i], d.ns_len[i], d.ns_dst[i] = s, l, t
    return d


def layout(descs, gap=48):
    """place the descriptors one after another, a sentinel gap between them; returns the arena size"""
    off = 64
    for d in descs:
        d.dst_off = off
        off += ((d.rows - 1) * d.ld_dst + d.cols) * PR.esz(d.dst_dt)
        off = (off + gap + 15) // 16 * 16
    return off + 64


def sentinel(n):
    return np.resize(SENTINEL, n)


class Table:
    def __init__(self, descs, master):
        self.descs, self.master = descs, np.asarray(master, dtype=np.float32)
        self.nbytes = layout(descs)
        self.pref = PR.tile_prefix(descs)
        self.ntiles = int(self.pref[-1])
        raw = np.frombuffer(bytes((L.PackDesc * len(descs))(*descs)), dtype=np.uint8).copy()
        self.descs_dev = torch.from_numpy(raw).cuda()
        self.pref_dev = torch.from_numpy(self.pref).cuda()
        self.tdesc_dev = torch.from_numpy(np.repeat(np.arange(len(descs), dtype=np.int32), np.diff(self.pref))).cuda()
        self.master_dev = torch.from_numpy(self.master).cuda()
        self.fill = sentinel(self.nbytes)
        PR.check_plan(descs, self.nbytes, [("master", 0, self.master.size)])

    def arena(self):
        return torch.from_numpy(self.fill.copy()).cuda()

    def run(self, arena, lo=0, hi=None, table=True):
        hi = self.ntiles if hi is None else hi
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if table is None:
            rc = L.load().cmpc_pack_weights(self.master_dev.data_ptr(), arena.data_ptr(), self.descs_dev.data_ptr(), self.pref_dev.data_ptr(),
                                            len(self.descs), self.ntiles, st)
        else:
            rc = L.load().cmpc_pack_weights_range(self.master_dev.data_ptr(), arena.data_ptr(), self.descs_dev.data_ptr(),
                                                  self.pref_dev.data_ptr(), self.tdesc_dev.data_ptr() if table else None, len(self.descs),
                                                  lo, hi, st)
        assert rc == 0, L.load().cmpc_last_error()
        torch.cuda.synchronize()
        return arena.cpu().numpy()

    def expected(self):
        return PR.expected_arena(self.descs, self.master, self.nbytes, fill=self.fill)

    def check(self, got, what=""):
        exp, written = self.expected()
        assert written[:64].sum() == 0 and written[-64:].sum() == 0
        PR.assert_arena_equal(got, exp, self.descs, what)


def segments(rng, n, ext, src_ext, align):
    """n segments inside [0, ext) with gaps between them (in increasing dst order), sources inside [0, src_ext)"""
    out, slot = [], ext // n
    for i in range(n):
        a = i * slot + int(rng.integers(0, max(1, slot // 4)))
        ln = int(rng.integers(max(1, slot // 3), max(2, slot - (a - i * slot))))
        ln = min(ln, src_ext)
        if align:
            a, ln = a // 4 * 4, max(4, ln // 4 * 4)
            if a + ln > (i + 1) * slot:
                ln = max(4, ((i + 1) * slot - a) // 4 * 4)
        s = int(rng.integers(0, src_ext - ln + 1))
        if align:
            s = s // 4 * 4
        out.append((s, ln, a))
    return out


def make_table(dt, tr, seed, shapes, align):
    """one descriptor per (Kp, Np, nks, nns) of `shapes`, sources packed into one master"""
    rng = np.random.default_rng(seed)
    descs, off = [], 0
    for (Kp, Np, nks, nns) in shapes:
        src_k, src_n = Kp + 5, Np + 3
        ld = (src_n + 3) // 4 * 4 + 4 if align else src_n + 4
        ks = segments(rng, nks, Kp, src_k, False)
        ns = segments(rng, nns, Np, min(src_n, ld), align)
        off += int(rng.integers(0, 3)) if not align else 0
        descs.append(desc(dt, tr, Kp, Np, ks, ns, off, ld, ld_pad=int(rng.choice([0, 8, 64]))))
        off += src_k * ld + 4
    return Table(descs, PR.stress_master(off + 8, seed))


# (Kp, Np, nks, nns): partial 64 x 128 tiles in both dimensions, every nks 1..4 and nns 1..5
SHAPES = [(8, 8, 1, 1), (64, 128, 1, 2), (72, 136, 2, 3), (136, 264, 3, 4), (200, 392, 4, 5), (16, 520, 2, 5), (328, 24, 4, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("align", [True, False], ids=["seg4", "seg1"])
@pytest.mark.parametrize("tr", [0, 1])
@pytest.mark.parametrize("dt", [0, 1, 2], ids=["f32", "bf16", "f16"])
def test_pack_matches_restatement(dt, tr, align):
    """many descriptors in one table; seg4: segment ends on multiples of 4 with 16-B aligned sources (the float4 path), seg1: segment
    ends and source offsets anywhere (element by element where a float4 would cross them)"""
    t = make_table(dt, tr, 100 + 10 * dt + tr + 3 * align, SHAPES, align)
    got = t.run(t.arena())
    t.check(got, f"dt {dt} tr {tr}")
    # the table lookup and the binary search over tile_prefix give the same bytes
    assert np.array_equal(t.run(t.arena(), table=False), got)
    assert np.array_equal(t.run(t.arena(), table=None), got)


@pytest.mark.gpu
@pytest.mark.parametrize("dt,tr", [(0, 0), (1, 1), (2, 1)])
def test_pack_large_descriptor(dt, tr):
    """one descriptor of 2048 x 1024 (plus partial tiles) beside small ones"""
    t = make_table(dt, tr, 7 + dt, [(8, 8, 1, 1), (2048 + 40, 1024 + 24, 2, 3), (64, 136, 1, 2)], True)
    t.check(t.run(t.arena()), "large")


@pytest.mark.gpu
@pytest.mark.parametrize("ld", [3, 5, 37])
@pytest.mark.parametrize("dt,tr", [(0, 0), (0, 1), (1, 1), (2, 0)])
def test_pack_unaligned_rows(dt, tr, ld):
    """master rows that are not 16-B aligned (the video parser's [500, 5]): every column of the row, nothing past it"""
    rng = np.random.default_rng(ld)
    descs, off = [], 0
    for (Kp, Np, nks) in ((64, 64, 1), (136, 8, 2), (200, 136, 3)):
        K = Kp - 9
        n = min(ld, Np)
        ks = segments(rng, nks, Kp, K, False)
        descs.append(desc(dt, tr, Kp, Np, ks, [(0, n, 0)] if ld < 8 or Np < 64 else [(0, 4, 0), (5, min(ld - 5, Np - 8), 8)], off, ld))
        off += K * ld + 1
    t = Table(descs, PR.stress_master(off, ld))
    t.check(t.run(t.arena()), f"ld {ld}")


@pytest.mark.gpu
@pytest.mark.parametrize("dt,tr", [(1, 1), (2, 0)])
def test_pack_ranges_split_the_table(dt, tr):
    """cmpc_pack_weights_range over split points, some in the middle of a descriptor: each range writes its own tiles and nothing else,
    and the ranges together give the full pack"""
    t = make_table(dt, tr, 31, SHAPES, False)
    exp, _ = t.expected()
    cuts = sorted({0, 1, int(t.pref[2]), int(t.pref[3]) + 1, int(t.pref[4]) + 3, int(t.pref[5]) - 1, t.ntiles - 1, t.ntiles})
    whole = t.arena()
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        got = t.run(t.arena(), lo, hi)
        m = PR.tile_mask(t.descs, range(lo, hi), t.nbytes)
        PR.assert_arena_equal(got, np.where(m, exp, t.fill), t.descs, f"tiles [{lo}, {hi})")
        t.run(whole, lo, hi)
    PR.assert_arena_equal(whole.cpu().numpy(), exp, t.descs, "union")
    assert np.array_equal(t.run(t.arena(), 5, 5), t.fill)          # an empty range launches nothing


@pytest.mark.gpu
def test_pack_conversions():
    """each stress value through every dtype, at a known position: the restatement's rounding is the kernel's"""
    x = np.concatenate([PR.STRESS, -PR.STRESS]).astype(np.float32)
    n = (x.size + 7) // 8 * 8
    master = np.zeros(n, dtype=np.float32)
    master[:x.size] = x
    for dt in (0, 1, 2):
        for tr in (0, 1):
            t = Table([desc(dt, tr, 8, n, [(0, 1, 0)], [(0, n, 0)], 0, n)], master)
            got, (exp, _) = t.run(t.arena()), t.expected()
            t.check(got, f"dt {dt} tr {tr}")
            if dt == 1:      # the ties, spelled out: 0x3F808000 -> 0x3F80 (even), 0x3F818000 -> 0x3F82 (odd rounds up)
                v = got[64:64 + 2 * n].view(np.uint16) if tr == 0 else got[64::2 * 8][:n] | (got[65::2 * 8][:n].astype(np.uint16) << 8)
                assert int(v[0]) == 0x3F80 and int(v[1]) == 0x3F82 and int(v[2]) == 0x3F81
            if dt == 2 and tr == 0:
                v = got[64:64 + 2 * n].view(np.float16)
                k = list(PR.STRESS.view(np.uint32)).index(np.float32(65519.99).view(np.uint32))
                assert v[k] == 65504 and np.isinf(v[k + 1]) and v[k + 1] > 0
