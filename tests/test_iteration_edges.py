"""The 256-thread routing and level-2 kernels on tiles crafted against their iteration size (tests/_iteration_edges.py).

A launch picks its forms in two places (xpng_amd/csrc/common.hpp): wide_form(items) selects the stream-per-lane rANS chains and
can be forced through the environment; small_blocks(items) = items > 2048 selects k_m1_streams<PXSZ, 256>, k_m2_streams<256> and
k_m2_dec_resid<256> and cannot.  Production pairs the wide chains with the 256-thread kernels; a forced-wide launch of a small
input pairs them with the 1024-thread ones.  The 256-thread form hands its serial state on every 1024 pixels, the other every
4096, so a hidden run, a zero-bit stretch or a tile end that sits on a multiple of 1024 meets a different piece of code there.

The CPU part proves from the oracle's planes and streams that every raster of the catalogue has the property in its name.  The
GPU part reaches the 256-thread form the way callers do - by the size of the launch - and runs the same rasters through the
other two pairings.  Every comparison is on bytes against the oracle; there is no tolerance and no timing."""
import numpy as np
import pytest

import _iteration_edges as E
from _kit import GUARD, SENTINEL, _upload, gpu, po
from test_steered import census

NL_NONE = E.NL_NONE
FORMATS = [(1, "rgba"), (1, "rgb"), (2, "rgb")]                   # (level, format)
# Tiles the oracle stores raw.  nl = 8 on every pixel is 24 bits per pixel in k (level 1) or three symbols of an alphabet of 256
# (level 2): with the block headers that is more than the 3 bytes per pixel of a raw RGB tile.  (RGBA: 4 bytes, so it is coded.)
RAW = {(nm, level) for level in (1, 2) for nm in E.names("rgb") if nm.startswith("one_context_8_")}


def _ch(fmt):
    return 4 if fmt == "rgba" else 3


def _runs(hidden):
    """[(first, last)] of the runs of True in a boolean vector"""
    edge = np.flatnonzero(np.diff(np.concatenate([[0], hidden.astype(np.int8), [0]])))
    return [(int(a), int(b) - 1) for a, b in zip(edge[::2], edge[1::2])]


def _block_sums(v, size):
    return [int(v[a:a + size].sum()) for a in range(0, len(v), size)]


@pytest.fixture(scope="module")
def planes(po):
    """name -> (nl plane, bits per pixel, pl per pixel, streams) from the oracle, for every raster built from a target; asserts
    on the way that the raster is one tile and that its nl plane is the target"""
    out = {}
    for fmt in ("rgba", "rgb"):
        for name in E.names(fmt):
            r = E.raster(name)
            h, w, ch = r.shape
            tt = po.tile_table(w, h, ch)
            assert tt == [(0, 0, w, h)], name
            pr, sums = po.choose_predictor(r, tt[0])
            assert pr & 3 == 0, (name, sums)                        # the predictor the generator built the residuals for
            p = po.m1_planes(r, tt[0], pr)
            T, _ = E.target(name)
            assert np.array_equal(p["nl"], T), (name, pr, np.flatnonzero(p["nl"] != T)[:4])
            nl = p["nl"].astype(np.int64)
            coded = nl != NL_NONE
            bits = np.where(coded, 3 * nl, 0)
            pl = np.zeros(len(nl), dtype=np.int64)                  # the context of every pixel: nl of the coded pixel before it
            idx = np.flatnonzero(coded)
            pl[idx[1:]] = nl[idx[:-1]]
            st = po.m1_streams(r, tt[0], p)
            assert [len(c) for c in st["ctx"]] == [int((coded & (pl == c)).sum()) for c in range(9)], name
            assert len(st["k"]) == -(-(8 * ch + int(bits.sum())) // 32), name   # the bit counts below are those of the stream k
            out[name] = (nl, bits, pl, st)
    return out


# ================================================================================================ CPU: the catalogue does what it claims
def test_every_raster_round_trips_and_is_coded(po):
    """One tile each; the oracle's decode_tiles of its encode_tiles gives the raster at every level of its format; an RGBA raster
    is its own normalize_rgba; and the tile is a coded one - its bytes depend on the routing - except the RGB rasters with nl = 8
    throughout, which no encoder can code below 3 bytes a pixel."""
    for level, fmt in FORMATS:
        for name in E.names(fmt, level):
            r = E.raster(name)
            h, w, ch = r.shape
            assert ch == _ch(fmt) and len(po.tile_table(w, h, ch)) == 1, name
            blob = po.encode_tiles(level, r)
            assert np.array_equal(po.decode_tiles(level, blob, w, h, ch), r), (name, level)
            assert (blob[3] == 0) == ((name, level) in RAW), (name, level, blob[3])
            if ch == 4:
                assert w >= 4 and h >= 4 and np.array_equal(po.normalize_rgba(r), r), name
                assert (r[r[..., 3] == 0] == 0).all(), name


def test_level2_extras_are_gray_and_single_colour(po):
    """Per size one gray tile and one single-colour tile: their workgroups leave k_m2_streams early, beside workgroups that do not."""
    extra = [nm for nm in E.names("rgb", 2) if nm not in set(E.names("rgb"))]
    assert len(extra) == 2 * len(E.SIZES)
    for name in extra:
        kinds = {b[0] for b in census(E.raster(name), 2)}
        assert ("gray" in kinds) if name.startswith("gray_") else (kinds == {"l2"}), (name, kinds)


def test_hidden_runs_begin_and_end_where_their_names_say(planes):
    """hidden_run_<k>_<kind>: exactly one NL_NONE run behind pixel 0, its ends at the pixels RUN_KINDS gives relative to 1024 k;
    the coded pixels on its two sides differ in nl (a wrong carry of the last coded nl across the run then moves a symbol to
    another context stream); `iter` and `iter_pm` hold a 1024-pixel block, aligned to 1024, of NL_NONE only and of zero bits,
    `wave` a whole 256-pixel wavefront's share, aligned to 256."""
    seen = set()
    for name in E.names("rgba"):
        _, meta = E.target(name)
        if meta["cls"] != "hidden_run":
            continue
        nl, bits, pl, _ = planes[name]
        k, kind = meta["k"], meta["kind"]
        runs = _runs(nl[1:] == NL_NONE)
        assert len(runs) == 1, (name, runs)
        first, last = runs[0][0] + 1, runs[0][1] + 1
        a, b = E.RUN_KINDS[kind]
        assert (first - 1024 * k, last - 1024 * k) == (a, b), (name, first, last)
        assert {"end_m1": last % 1024 == 1023, "end_0": last % 1024 == 0, "end_p1": last % 1024 == 1,
                "begin_m1": first % 1024 == 1023, "begin_0": first % 1024 == 0, "begin_p1": first % 1024 == 1,
                "wave": first % 256 == 0 and last - first == 255, "iter": first % 1024 == 0 and last - first == 1023,
                "iter_pm": first % 1024 == 1023 and last - first == 1025}[kind], name
        assert nl[first - 1] != NL_NONE
        if last + 1 < len(nl):
            assert nl[last + 1] != NL_NONE and nl[last + 1] != nl[first - 1], name
            assert pl[last + 1] == nl[first - 1], name                 # the context of the pixel behind the run comes from before it
        if kind in ("iter", "iter_pm"):
            i0 = 1024 * k
            assert (nl[i0:i0 + 1024] == NL_NONE).all() and _block_sums(bits, 1024)[k] == 0, name
        seen.add((kind, k))
    for kind in E.RUN_KINDS:                                             # every kind, on a boundary of the 256-thread form alone and on 4096
        assert {k for (kd, k) in seen if kd == kind} >= {1, 4}, kind


def test_hidden_tails_end_the_tile_inside_a_run_and_a_ragged_dword(planes):
    mods = set()
    for name in E.names("rgba"):
        _, meta = E.target(name)
        if meta["cls"] != "hidden_tail":
            continue
        nl = planes[name][0]
        runs = _runs(nl[1:] == NL_NONE)
        assert len(runs) == 1 and runs[0][1] + 1 == len(nl) - 1 and runs[0][1] - runs[0][0] + 1 == E.TAIL, (name, runs)
        mods.add(len(nl) % 4)
    assert mods == {0, 1, 2, 3}


def test_bitrate_steps_switch_at_the_boundaries_and_fill_whole_iterations(planes):
    """bitrate_steps_m1 / _p1: nl is 0 or 8 and changes exactly one pixel before / behind every multiple of 1024.
    bitrate_steps_r<r>: every whole 1024-pixel block behind the first holds 24576 bits (odd blocks) or none (even blocks), the
    4096-pixel blocks their sums, and the bit cursor (the raw first pixel included) is r mod 32 at every multiple of 1024: where
    r is not 0, the partial last word crosses the zero-bit iterations unchanged."""
    residues = {"rgba": set(), "rgb": set()}
    for fmt in ("rgba", "rgb"):
        for name in E.names(fmt):
            _, meta = E.target(name)
            if meta["cls"] != "bitrate_steps":
                continue
            nl, bits, _, _ = planes[name]
            n, d = len(nl), meta["shift"]
            if d:
                assert set(nl[1:].tolist()) <= {0, 8}, name
                want = [1024 * k + d for k in range(1, n // 1024 + 2) if 1 < 1024 * k + d < n]
                assert (np.flatnonzero(nl[2:] != nl[1:-1]) + 2).tolist() == want, name
                continue
            r = meta["residue"]
            ph = E.phase_pixels(r, _ch(fmt))
            b1 = _block_sums(bits, 1024)
            assert b1[0] == 3 * sum(ph) and nl[1:1 + len(ph)].tolist() == ph, name
            for j in range(1, len(b1)):
                size = min(1024, n - 1024 * j)
                assert b1[j] == (24 * size if j & 1 else 0), (name, j)
            assert _block_sums(bits, 4096) == [sum(b1[a:a + 4]) for a in range(0, len(b1), 4)], name
            if n >= 4096:
                assert _block_sums(bits, 4096)[0] == 3 * sum(ph) + 2 * 24576, name
            cursor = 8 * _ch(fmt) + np.concatenate([[0], np.cumsum(bits)])    # the bit cursor in front of every pixel
            for j in range(1, -(-n // 1024)):
                assert cursor[1024 * j] & 31 == r, (name, j)
                residues[fmt].add(r)
            if n > 3072:                                                       # a zero-bit iteration behind a full one
                assert b1[1] == 24576 and b1[2] == 0, name
    assert residues == {"rgba": set(E.RESIDUES), "rgb": set(E.RESIDUES)}


def test_one_context_fills_a_wavefront_and_the_cycle_visits_every_transition(planes):
    """one_context_<v>: every coded pixel has nl v, so behind pixel 1 every pixel appends to context stream v: each whole 256-pixel
    wavefront adds 256 symbols to one stream (the 10-bit count field of the packed scan holds 256).  cycle: nl = i mod 9."""
    for fmt in ("rgba", "rgb"):
        for name in E.names(fmt):
            _, meta = E.target(name)
            nl, _, pl, st = planes[name]
            n = len(nl)
            if meta["cls"] == "one_context":
                v = meta["v"]
                assert (nl[1:] == v).all() and pl[1] == 0 and (pl[2:] == v).all(), name
                assert n >= 1023
                for a in range(256, n - 255, 256):                      # the whole wavefronts behind the first
                    assert (pl[a:a + 256] == v).all() and (nl[a:a + 256] != NL_NONE).all(), (name, a)
                assert len(st["ctx"][v]) == (n - 1 if v == 0 else n - 2), name
            elif meta["cls"] == "cycle":
                assert np.array_equal(nl[1:], np.arange(1, n) % 9), name
                assert [len(c) for c in st["ctx"]] == [int((np.arange(1, n - 1) % 9 == c).sum()) + (c == 0) for c in range(9)], name


def test_class_steps_change_class_at_the_boundaries_and_write_every_level2_form(planes, po):
    """class_steps_<shift>: stretches of 512 pixels of one nl each; 1|2, 7|0, 4|1, 5|8 and 6|2 meet at 1024 k + shift.  At level 2
    the larger tiles write class 1 (packed at 3 bits), class 2 (6 bits), every class 3 .. 8 (3 bytes) and pixels of nl 0, which
    emit no class symbol."""
    for name in E.names("rgb"):
        _, meta = E.target(name)
        if meta["cls"] != "class_steps":
            continue
        nl = planes[name][0]
        n, d = len(nl), meta["shift"]
        change = (np.flatnonzero(nl[2:] != nl[1:-1]) + 2).tolist()
        assert change == [c for c in range(512 + d, n, 512) if c > 1], name
        pairs = {(int(nl[c - 1]), int(nl[c])) for c in change if (c - d) % 1024 == 0}
        assert pairs == set([(1, 2), (7, 0), (4, 1), (5, 8), (6, 2)][: len(pairs)]) and (n < 1100 or pairs), (name, pairs)
        if n >= 5120:
            got = census(E.raster(name), 2)
            assert ("l2_pr", 0) in got and (nl[1:] == 0).any(), name
            for c in range(1, 9):
                assert any(b[0] == "l2_cls" and b[1] == c and b[2] != 0 for b in got), (name, c, sorted(got, key=str))


def test_catalogue_spans_both_iteration_sizes_and_fills_a_launch(planes):
    """In every class some size takes different numbers of iterations in the two forms; and every (level, format) list is longer
    than 2048 / spt images, so a launch of the list selects the 256-thread kernels by itself."""
    differs = {}
    for fmt in ("rgba", "rgb"):
        for name in E.names(fmt):
            n = len(planes[name][0])
            cls = (fmt, E.target(name)[1]["cls"])
            differs[cls] = differs.get(cls, False) or -(-n // E.IT_SMALL) != -(-n // E.IT_BIG)
    assert set(differs) == {("rgba", c) for c in ("hidden_run", "hidden_tail", "bitrate_steps", "one_context", "cycle")} | \
        {("rgb", c) for c in ("bitrate_steps", "one_context", "cycle", "class_steps")} and all(differs.values()), differs
    for level, fmt in FORMATS:
        names = E.names(fmt, level)
        assert len(names) == len(set(names)) and len(names) * E.SPT[(level, fmt)] > 2048, (level, fmt, len(names))
        for (w, h) in E.BATCH_SIZES:
            assert len(E.of_size(fmt, level, w, h)) >= 20, (level, fmt, w, h)


# ================================================================================================ GPU: bit-exact against the oracle
_ORACLE = {}


def _blob(po, name, level):
    """The oracle's tile blob of a catalogue raster (computed once, shared, never changed)."""
    if (name, level) not in _ORACLE:
        _ORACLE[(name, level)] = po.encode_tiles(level, E.raster(name))
    return _ORACLE[(name, level)]


def _first_wrong_stream(gpu, po, name):
    """Where a single-image Context first differs from the oracle on a level-1 raster: planes, context streams, k, rANS blocks.  It
    runs the 1024-thread kernels, so `None` here beside a failure of a large launch puts the fault in the 256-thread form alone."""
    import torch
    r = E.raster(name)
    h, w, ch = r.shape
    ctx = gpu.Context(w, h, ch)
    try:
        d_r = torch.from_numpy(r.copy()).cuda()
        d_b = torch.zeros(ctx.blob_bound() + 64, dtype=torch.uint8, device="cuda")
        t = ctx.tiles()[0]
        pr, _ = po.choose_predictor(r, t)
        p = po.m1_planes(r, t, pr)
        ctx.encode_device(1, d_r.data_ptr(), d_b.data_ptr())
        for k in ("nl", "r", "g", "b"):
            if not np.array_equal(ctx.fetch(k, 0), p[k]):
                return "plane " + k
        st = po.m1_streams(r, t, p)
        for c in range(9):
            if not np.array_equal(ctx.fetch(10 + c, 0), st["ctx"][c]):
                return f"context stream {c}"
        if not np.array_equal(ctx.fetch("k", 0).view(np.uint32), st["k"]):
            return "bit stream k"
        for c in range(9):
            if ctx.fetch(20 + c, 0).tobytes() != po.rans2_encode(st["F"][c], 9, st["ctx"][c], 12):
                return f"rANS block {c}"
        return None
    finally:
        ctx.close()


def _explain(gpu, po, name, level, form):
    if level != 1:
        return (name, level, form)
    return (name, level, form, "single-image context (1024-thread form): first difference", _first_wrong_stream(gpu, po, name))


def _encode_mixed(gpu, po, ctx, level, names, form):
    """encode_batch of the named rasters: blob i is the oracle's, nothing written behind the returned length"""
    import torch
    d_r = [torch.from_numpy(E.raster(nm).copy()).cuda() for nm in names]
    d_b = [torch.full((ctx.blob_bound(i) + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for i in range(ctx.nimg)]
    lens = ctx.encode_batch(level, [t.data_ptr() for t in d_r], [t.data_ptr() for t in d_b])
    torch.cuda.synchronize()
    for nm, t, ln in zip(names, d_b, lens):
        got, want = t.cpu().numpy(), _blob(po, nm, level)
        if ln != len(want) or got[:ln].tobytes() != want:
            pytest.fail("encode: %r" % (_explain(gpu, po, nm, level, form),))
        assert (got[ln:] == SENTINEL).all(), (nm, level, form, "bytes behind the returned length written")


def _decode_mixed(ctx, po, level, names, form):
    """decode_batch of the oracle's blobs: the rasters, nothing written behind them"""
    import torch
    blobs = [_blob(po, nm, level) for nm in names]
    d_o = [torch.full((E.raster(nm).size + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for nm in names]
    d_b = _upload(blobs)
    ctx.decode_batch(level, [t.data_ptr() for t in d_b], [len(b) for b in blobs], [t.data_ptr() for t in d_o])
    assert ctx.decode_status() == 0, (level, form)
    torch.cuda.synchronize()
    for nm, t in zip(names, d_o):
        r, got = E.raster(nm), t.cpu().numpy()
        assert np.array_equal(got[: r.size].reshape(r.shape), r), ("decode", nm, level, form)
        assert (got[r.size:] == SENTINEL).all(), ("decode", nm, level, form, "bytes behind the raster written")


def _mixed(gpu, names, fmt):
    return gpu.MixedContext([(E.raster(nm).shape[1], E.raster(nm).shape[0]) for nm in names], _ch(fmt))


@pytest.mark.gpu
@pytest.mark.parametrize("first", ["decode", "encode"])
@pytest.mark.parametrize("level,fmt", FORMATS)
def test_whole_catalogue_in_one_mixed_launch_takes_the_256_thread_kernels(gpu, po, level, fmt, first):
    """Every raster of a format in one MixedContext: tiles x streams > 2048, so the launch takes the wide chains and
    k_m1_streams<PXSZ, 256> / k_m2_streams<256> / k_m2_dec_resid<256> by itself, as production does.  Blobs and pixels against the
    oracle, sentinels behind both, on one context in either order."""
    names = E.names(fmt, level)
    ctx = _mixed(gpu, names, fmt)
    try:
        assert ctx.n_tiles == len(names) and ctx.n_tiles * E.SPT[(level, fmt)] > 2048
        for step in (first, "encode" if first == "decode" else "decode"):
            if step == "encode":
                _encode_mixed(gpu, po, ctx, level, names, "wide + 256, natural")
            else:
                _decode_mixed(ctx, po, level, names, "wide + 256, natural")
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["XPNG_NARROW_RANS", "XPNG_WIDE_RANS"])
@pytest.mark.parametrize("level,fmt", FORMATS)
def test_the_same_rasters_on_the_1024_thread_kernels_with_either_chains(gpu, po, monkeypatch, level, fmt, form):
    """The catalogue in chunks of at most 2048 / spt images, so that small_blocks() is false, with the narrow and with the forced
    wide chains: narrow + 1024, wide + 1024 and (the test above) wide + 256 meet the same rasters, and a failure names its form."""
    monkeypatch.setenv(form, "1")
    names, spt = E.names(fmt, level), E.SPT[(level, fmt)]
    per = 2048 // spt
    for a in range(0, len(names), per):
        chunk = names[a:a + per]
        ctx = _mixed(gpu, chunk, fmt)
        try:
            assert ctx.n_tiles * spt <= 2048
            what = ("narrow" if form == "XPNG_NARROW_RANS" else "wide") + " + 1024, forced"
            _encode_mixed(gpu, po, ctx, level, chunk, what)
            _decode_mixed(ctx, po, level, chunk, what)
        finally:
            ctx.close()


def _uniform_batch(gpu, po, level, names, B):
    """encode_device_batch and decode_device_batch over B images cycling through the named rasters of one size: the blobs are the
    oracle's, the pixels the rasters', sentinels behind both.  Returns the blobs."""
    import torch
    rasters = [E.raster(nm) for nm in names]
    wants = [_blob(po, nm, level) for nm in names]
    h, w, ch = rasters[0].shape
    k = len(rasters)
    ctx = gpu.Context(w, h, ch, batch=B)
    try:
        assert ctx.n_tiles == 1
        d_src = [torch.from_numpy(r.copy()).cuda() for r in rasters]
        d_b = [torch.full((ctx.blob_bound() + 64,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(B)]
        lens = ctx.encode_device_batch(level, [d_src[i % k].data_ptr() for i in range(B)], [t.data_ptr() for t in d_b])
        got = [t.cpu().numpy() for t in d_b]
        for i in range(B):
            if lens[i] != len(wants[i % k]) or got[i][: lens[i]].tobytes() != wants[i % k]:
                pytest.fail("encode, image %d of %d: %r" % (i, B, _explain(gpu, po, names[i % k], level, "uniform batch")))
            assert (got[i][lens[i]:] == SENTINEL).all(), (level, i, B)
        nbytes = w * h * ch
        d_o = [torch.full((nbytes + 64,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(B)]
        ctx.decode_device_batch(level, [t.data_ptr() for t in d_b], lens, None, [t.data_ptr() for t in d_o])
        assert ctx.decode_status() == 0
        for i in range(B):
            assert torch.equal(d_o[i][:nbytes], d_src[i % k].reshape(-1)), ("decode", names[i % k], level, i, B)
            assert bool((d_o[i][nbytes:] == SENTINEL).all()), (level, i, B)
        return [g[:n].tobytes() for g, n in zip(got, lens)]
    finally:
        ctx.close()


THRESHOLD = {(1, "rgba"): 205, (1, "rgb"): 228, (2, "rgb"): 121}  # the smallest B with B * spt > 2048 (no spt divides 2048)


@pytest.mark.gpu
@pytest.mark.parametrize("size", E.BATCH_SIZES)
@pytest.mark.parametrize("level,fmt", FORMATS)
def test_uniform_batches_on_both_sides_of_the_threshold(gpu, po, level, fmt, size):
    """A Context(w, h, ch, batch=B) with the catalogue's rasters of that size cycling through its images.  At the smallest B with
    more than 2048 items the launch selects the wide chains and the 256-thread kernels by itself: 1025 pixels are two of their
    iterations and one of the 1024-thread form's, 4097 pixels five and two.  B - 1 images are the largest launch at or below 2048
    items: narrow chains and 1024-thread kernels, no switch set.  The oracle's bytes on both sides, hence the same."""
    B, spt = THRESHOLD[(level, fmt)], E.SPT[(level, fmt)]
    assert (B - 1) * spt <= 2048 < B * spt
    names = E.of_size(fmt, level, *size)
    below = _uniform_batch(gpu, po, level, names, B - 1)
    above = _uniform_batch(gpu, po, level, names, B)
    assert above[: B - 1] == below
