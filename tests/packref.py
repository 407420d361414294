"""Restatement of pack_kernel (include/cmpc.h, cmpc_pack_weights): the bytes a descriptor table writes into the operand arena, and
the plan checks every table must pass (the kernel's preconditions, destinations inside the arena without overlap, sources inside one
parameter).  numpy only: used by the CPU plan tests and by the GPU tests that compare the kernel's bytes with these."""
import ctypes

import numpy as np

DT_F32, DT_BF16, DT_F16 = 0, 1, 2


def esz(dt):
    return 4 if dt == DT_F32 else 2


def bf16_bits(x):
    """float32 -> bfloat16 bits, round to nearest even; NaN stays NaN with its sign (quietened)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    nan = np.isnan(x)
    r[nan] = ((u[nan] >> np.uint32(16)) | np.uint32(0x0040)).astype(np.uint16)
    return r


def f16_bits(x):
    """float32 -> float16 bits, numpy's conversion: round to nearest even, overflow to inf, NaN stays NaN with its sign."""
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(x, dtype=np.float32).astype(np.float16).view(np.uint16)


def to_bytes(blk, dt):
    """[rows, cols] float32 -> [rows, cols * esz(dt)] uint8 as the kernel stores it"""
    blk = np.ascontiguousarray(blk, dtype=np.float32)
    bits = blk.view(np.uint32) if dt == DT_F32 else (bf16_bits(blk) if dt == DT_BF16 else f16_bits(blk))
    return bits.view(np.uint8).reshape(blk.shape[0], -1)


def kn(d):
    """(Kp, Np) of a descriptor: K = master rows, N = master columns of the padded block"""
    return (d.cols, d.rows) if d.transpose else (d.rows, d.cols)


def segs(d):
    return ([(d.ks_src[i], d.ks_len[i], d.ks_dst[i]) for i in range(d.nks)],
            [(d.ns_src[j], d.ns_len[j], d.ns_dst[j]) for j in range(d.nns)])


def emulate_pack(d, master):
    """float32 block [rows, cols] one descriptor writes: master[src_off + (ks_src + k - ks_dst) * ld_src + ns_src + n - ns_dst] inside a
    segment pair, 0 in the padding"""
    Kp, Np = kn(d)
    blk = np.zeros((Kp, Np), dtype=np.float32)
    ks, ns = segs(d)
    for (ksrc, kl, kd) in ks:
        for (nsrc, nl, nd) in ns:
            idx = np.arange(ksrc, ksrc + kl)[:, None] * d.ld_src + np.arange(nsrc, nsrc + nl)[None, :]
            blk[kd:kd + kl, nd:nd + nl] = master[d.src_off + idx]
    return blk.T if d.transpose else blk


def _view(buf, d):
    e = esz(d.dst_dt)
    return np.lib.stride_tricks.as_strided(buf[d.dst_off:], shape=(d.rows, d.cols * e), strides=(d.ld_dst * e * buf.itemsize, buf.itemsize),
                                           writeable=True)


def expected_arena(descs, master, arena_bytes, fill=None):
    """(bytes, written): the arena after packing `descs` from `master` (uint8 [arena_bytes], starting from `fill` or zeros), and the
    mask of the bytes a descriptor writes"""
    out = np.zeros(arena_bytes, dtype=np.uint8) if fill is None else np.array(fill, dtype=np.uint8, copy=True)
    written = np.zeros(arena_bytes, dtype=bool)
    master = np.asarray(master, dtype=np.float32)
    for d in descs:
        _view(out, d)[...] = to_bytes(emulate_pack(d, master), d.dst_dt)
        _view(written, d)[...] = True
    return out, written


def assert_arena_equal(got, exp, descs, what=""):
    """Every byte equal.  The one freedom: where the restatement holds a NaN, the kernel's NaN may carry another payload, but it must be
    a NaN of the same sign."""
    got, exp = np.asarray(got, dtype=np.uint8), np.asarray(exp, dtype=np.uint8)
    bad = np.flatnonzero(got != exp)
    if bad.size == 0:
        return
    starts = np.array([d.dst_off for d in descs], dtype=np.int64)
    order = np.argsort(starts)
    for b in bad[:4096]:
        i = order[max(np.searchsorted(starts[order], b, side="right") - 1, 0)]
        d = descs[i]
        e = esz(d.dst_dt)
        rel = b - d.dst_off
        r, c = divmod(rel, d.ld_dst * e)
        ok = False
        if 0 <= r < d.rows and c < d.cols * e:
            o = b - (rel % e)
            ge, ee = got[o:o + e], exp[o:o + e]
            if e == 4:
                gv, ev = ge.view(np.float32)[0], ee.view(np.float32)[0]
                gs, es_ = ge.view(np.uint32)[0] >> 31, ee.view(np.uint32)[0] >> 31
            else:
                gu, eu = int(ge.view(np.uint16)[0]), int(ee.view(np.uint16)[0])
                if d.dst_dt == DT_BF16:
                    gv, ev = np.float32(np.uint32(gu << 16).view(np.float32)), np.float32(np.uint32(eu << 16).view(np.float32))
                else:
                    gv, ev = np.uint16(gu).view(np.float16), np.uint16(eu).view(np.float16)
                gs, es_ = gu >> 15, eu >> 15
            ok = bool(np.isnan(ev) and np.isnan(gv) and gs == es_)
        assert ok, (f"{what}: byte {b} (descriptor {i}, row {r}, byte {c} of the row, dtype {d.dst_dt}, transpose {d.transpose}): "
                    f"got {got[b]:#04x}, expected {exp[b]:#04x}; {bad.size} bytes differ")


def row_intervals(descs):
    """[n, 2] byte intervals [start, end) of every destination row of every descriptor, and the descriptor index of each"""
    st, en, ix = [], [], []
    for i, d in enumerate(descs):
        e = esz(d.dst_dt)
        s = d.dst_off + np.arange(d.rows, dtype=np.int64) * d.ld_dst * e
        st.append(s); en.append(s + d.cols * e); ix.append(np.full(d.rows, i))
    return np.concatenate(st), np.concatenate(en), np.concatenate(ix)


def check_plan(descs, arena_bytes, params):
    """params: [(name, element offset, element count)] of the master buffer (cmpc_param_info).  Asserts the kernel's preconditions
    (include/cmpc.h) for every descriptor, every destination inside the arena, no two destinations overlapping, and every source
    rectangle inside one parameter."""
    poffs = np.array([o for _, o, _ in params], dtype=np.int64)
    order = np.argsort(poffs)
    for i, d in enumerate(descs):
        e = esz(d.dst_dt)
        Kp, Np = kn(d)
        assert d.dst_dt in (DT_F32, DT_BF16, DT_F16) and d.transpose in (0, 1), i
        assert d.cols % (8 if d.transpose else 4) == 0 and d.rows >= 1 and d.cols >= 1, (i, d.rows, d.cols)
        assert d.ld_dst >= d.cols and (d.ld_dst * e) % 16 == 0 and d.dst_off % 16 == 0, (i, d.ld_dst, d.dst_off)
        assert d.dst_off >= 0 and d.dst_off + ((d.rows - 1) * d.ld_dst + d.cols) * e <= arena_bytes, (i, "outside the arena")
        assert 1 <= d.nks <= 4 and 1 <= d.nns <= 5, i
        ks, ns = segs(d)
        for name, sg, ext in (("K", ks, Kp), ("N", ns, Np)):
            cover = np.zeros(ext, dtype=np.int32)
            for (s, l, t) in sg:
                assert s >= 0 and l >= 1 and 0 <= t and t + l <= ext, (i, name, (s, l, t), ext)
                cover[t:t + l] += 1
            assert cover.max() <= 1, (i, name, "segments overlap in the destination")
        for (s, l, _) in ns:
            assert s + l <= d.ld_src, (i, "N segment past the master row", (s, l), d.ld_src)
        lo = d.src_off + min(s for s, _, _ in ks) * d.ld_src + min(s for s, _, _ in ns)
        hi = d.src_off + max(s + l - 1 for s, l, _ in ks) * d.ld_src + max(s + l - 1 for s, l, _ in ns)
        j = order[np.searchsorted(poffs[order], lo, side="right") - 1]
        name, po, pc = params[j]
        assert po <= lo and hi < po + pc, (i, "source outside one parameter", name, (lo, hi), (po, po + pc))
    st, en, _ = row_intervals(descs)
    o = np.argsort(st, kind="stable")
    st, en = st[o], en[o]
    assert np.all(st[1:] >= en[:-1]), "two descriptors write the same bytes"


def check_operands(descs, ops):
    """ops: {key: (byte offset, dt, rows, ld)}.  Every operand's bytes are covered exactly by descriptors of its dtype, and the
    descriptors write nothing else (the totals agree, so an operand missing from `ops` is caught)."""
    st, en, ix = row_intervals(descs)
    o = np.argsort(st, kind="stable")
    st, en, ix = st[o], en[o], ix[o]
    total = 0
    for key, (off, dt, rows, ld) in ops.items():
        size = rows * ld * esz(dt)
        total += size
        a, b = np.searchsorted(st, off), np.searchsorted(st, off + size)
        assert b > a and st[a] == off and en[b - 1] == off + size and np.all(st[a + 1:b] == en[a:b - 1]), (key, "not covered exactly")
        assert all(descs[i].dst_dt == dt for i in np.unique(ix[a:b])), (key, "descriptor dtype")
    assert int((en - st).sum()) == total, ("descriptor bytes", int((en - st).sum()), "operand bytes", total)


def tile_prefix(descs):
    pref = np.zeros(len(descs) + 1, dtype=np.int32)
    for i, d in enumerate(descs):
        Kp, Np = kn(d)
        pref[i + 1] = pref[i] + ((Kp + 63) // 64) * ((Np + 127) // 128)
    return pref


# ---- the plans of a cmpc_create handle ----------------------------------------------------------------------------------------
MODELS = {"CMPC_model": (0, 0), "CMPCv5_BiLSTM_model": (1, 0), "CMPCv5_BiLSTM_HSV_model": (1, 1), "CMPCv5_model": (3, 0),
          "CMPCv5_HSV_model": (3, 1), "CMPC_video_mm_tgraph_allvec": (2, 0)}


def operand_keys(model, conv5=False):
    """the keys plan_operands (engine.hip) creates for a model code"""
    v5, bilstm, vid = model in (1, 3), model == 1, model == 2
    keys = []

    def lin(k, fwd=True, bwd=True):
        keys.extend(([k + ".t"] if fwd else []) + ([k + ".n"] if bwd else []))
    for k in (["lstm_fw", "lstm_bw"] if bilstm else ["lstm"]):
        lin(k)
        keys.append(k + ".b")
    if bilstm:
        lin("wfeat")
    lin("parse1"); lin("parse2")
    levels = ["c5", "c4"] if v5 else ["c5", "c4", "c3"]
    for lv in levels:
        lin(f"lat_{lv}", True, conv5)
    for lv in levels:
        keys += [f"mutan_{lv}.t", f"mutan_{lv}.n", f"mlang_{lv}.t", f"mlang_{lv}.n", f"mutan_{lv}.b", f"mlang_{lv}.b"]
        for k in ("wtrans", "t2", "gupd", "fus", "fusl"):
            lin(f"{k}_{lv}")
        if vid:
            lin(f"fussp_{lv}", True, False)
            for k in ("tgv", "tgl", "tgq", "tgk", "tgu", "mmt", "ctxt"):
                lin(f"{k}_{lv}")
    for x in (["c4", "c5", "c4_2", "c5_2"] if v5 else ["c3", "c4", "c5", "c3_2", "c4_2", "c5_2"]):
        for k in ("key", "query", "gv"):
            lin(f"{k}_{x}")
        for f in (["f1"] if v5 else ["f1", "f2"]):
            lin(f"lfeat_{x}_{f}"); lin(f"tfeat_{x}_{f}")
    lin("clstm")
    if v5:
        for k in ("aspp0", "aspp1", "aspp2", "aspp3", "aspp_img", "aspp_cat", "aspp_catl"):
            lin(k)
        lin("dec_low", True, False)
        lin("dec1"); lin("dec2")
    return keys


def handle_plan(lib, PackDesc, h):
    """(descs, arena_bytes, params, stage0_ndesc) of a handle, through cmpc_plan_info / cmpc_param_info"""
    descs, nd, ab, wb, s0 = ctypes.POINTER(PackDesc)(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
    assert lib.cmpc_plan_info(h, ctypes.byref(descs), ctypes.byref(nd), ctypes.byref(ab), ctypes.byref(wb), ctypes.byref(s0)) == 0
    ds = [PackDesc.from_buffer_copy(bytes(descs[i])) for i in range(nd.value)]
    params = []
    name, off, rank, shape = ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_int(), (ctypes.c_int64 * 4)()
    for i in range(lib.cmpc_param_count(h)):
        assert lib.cmpc_param_info(h, i, ctypes.byref(name), ctypes.byref(off), ctypes.byref(rank), ctypes.byref(shape)) == 0
        params.append((name.value.decode(), off.value, int(np.prod([shape[k] for k in range(rank.value)]))))
    return ds, ab.value, params, s0.value


def handle_operands(lib, h, keys):
    out = {}
    bo, dt, rows, ld = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for k in keys:
        assert lib.cmpc_operand_info(h, k.encode(), ctypes.byref(bo), ctypes.byref(dt), ctypes.byref(rows), ctypes.byref(ld)) == 0, \
            (k, lib.cmpc_last_error())
        out[k] = (bo.value, dt.value, rows.value, ld.value)
    return out


def tile_mask(descs, tiles, arena_bytes):
    """bytes written by the 64 (k) x 128 (n) tiles `tiles` (global tile indices, cmpc_pack_weights_range)"""
    pref = tile_prefix(descs)
    m = np.zeros(arena_bytes, dtype=bool)
    for gt in tiles:
        i = int(np.searchsorted(pref, gt, side="right") - 1)
        d = descs[i]
        Kp, Np = kn(d)
        tn = (Np + 127) // 128
        t = gt - pref[i]
        k0, n0 = (t // tn) * 64, (t % tn) * 128
        v = _view(m, d)
        e = esz(d.dst_dt)
        if d.transpose:
            v[n0:min(n0 + 128, Np), k0 * e:min(k0 + 64, Kp) * e] = True
        else:
            v[k0:min(k0 + 64, Kp), n0 * e:min(n0 + 128, Np) * e] = True
    return m


# masters that stress the conversions: bf16 ties to even / to odd and just past them, values around the f16 maximum (65504; 65520 is
# the first that rounds to inf), f16 subnormals and the subnormal tie, signed zeros, infinities and quiet NaNs of both signs
STRESS = np.concatenate([
    np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F817FFF, 0xBF808000, 0xBF818000, 0x7F7FFFFF, 0x00008000, 0x00018000],
             dtype=np.uint32).view(np.float32),
    np.array([65504.0, 65519.99, 65520.0, 65536.0, -65519.99, -65520.0, 1e6, 2.0 ** -24, 3 * 2.0 ** -25, 2.0 ** -25, 2.0 ** -15,
              -2.0 ** -24, 1e-8, 0.0, -0.0, np.inf, -np.inf], dtype=np.float32),
    np.array([0x7FC00000, 0xFFC00000], dtype=np.uint32).view(np.float32)])


def stress_master(n, seed):
    """n float32: normal values with every STRESS value placed at many positions"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n).astype(np.float32)
    pos = rng.choice(n, size=min(n, max(len(STRESS), n // 8)), replace=False)
    x[pos] = STRESS[np.arange(pos.size) % len(STRESS)]
    return x
