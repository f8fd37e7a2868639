"""The alpha reconstruction of the level-1 decode on crafted alpha planes (tests/_alpha_heads.py).

An RGBA tile's alpha is rebuilt by one of two hand-written forms (xpng_amd/csrc/m1_decode.hpp, decode_m1_plan):
  folded   k_dec_resid<4, THREADS, true>: every tile of the launch at least 4 px wide - every file an encoder writes;
  plane    k_dec_alpha<THREADS> then k_dec_resid<4, THREADS, false>: a tile under 4 px wide, or XPNG_NO_ALPHA_FOLD in the probes build;
THREADS is 1024 with the narrow rANS chains and 256 with the wide ones (more than 2048 (tile, stream) items, or XPNG_WIDE_RANS).

The CPU part proves from the oracle that every raster of the catalogue is one coded tile whose alpha symbols give its alpha plane
by the plain rule, takes a census of what the catalogue puts where in the walk of either workgroup size, and shows that three
wrong rules give other planes.  The GPU part decodes the oracle's blobs with all four kernel pairings and compares bytes; there is
no tolerance and no timing.  Every buffer a decode writes has 0xA5 bytes behind it that must stay; every decode's status is 0
(the host call api.decode_tiles turns any other status into an XpngError)."""
import fnmatch
import os

import numpy as np
import pytest

import _alpha_heads as A
from _hostile import tile_m1, v2_blk0, v2_blk1
from _kit import GUARD, SENTINEL, _upload, gpu, po  # noqa: F401  (fixtures)
from _rans_tables import sym_of_delta
from xpng_amd import api


# ================================================================================================ CPU
@pytest.fixture(scope="module")
def symbols(po):
    """name -> (a0, the alpha symbols of pixels 1 .. n - 1) from the oracle's planes (computed once, shared, never changed)"""
    out = {}
    for name in A.names():
        r = A.raster(name)
        h, w, _ = r.shape
        tt = po.tile_table(w, h, 4)
        assert tt == [(0, 0, w, h)], name
        pr, _ = po.choose_predictor(r, tt[0])
        sy = po.m1_planes(r, tt[0], pr)["a"][1:].copy()
        sy.setflags(write=False)
        out[name] = (int(r[0, 0, 3]), sy)
    return out


_ORACLE = {}


def _blob(po, name):
    """The oracle's tile blob of a catalogue raster (computed once, shared, never changed)."""
    if name not in _ORACLE:
        _ORACLE[name] = po.encode_tiles(1, A.raster(name))
    return _ORACLE[name]


def test_sizes_are_the_ones_the_walk_needs():
    W = [w for w, _ in A.SIZES]
    N = [w * h for w, h in A.SIZES]
    assert {4, 5, 6, 7, 63, 64, 65} <= set(W)
    assert {w % 4 for w in W if w > 256} == {0, 1, 2, 3}
    assert any(1024 < w <= 4096 for w in W) and any(w > 4096 for w in W)
    assert any(w < 8 and 256 < h <= 1024 for w, h in A.SIZES) and any(w < 8 and h > 1024 for w, h in A.SIZES)
    assert any(1024 < n <= 4096 for n in N) and any(n > 4096 for n in N) and {n % 4 for n in N} == {0, 1, 2, 3}
    assert all(w >= 4 and h >= 4 and w * h <= 30000 for w, h in A.SIZES)
    assert set(A.BATCH_SIZES) <= set(A.SIZES)
    nm = A.names()
    assert len(nm) == len(set(nm)) and {A.parse(x)[0] for x in nm} == set(A.KINDS)
    mixed = A.mixed_names()
    assert len(mixed) * A.SPT > 2048 and set(mixed) == set(nm)


def test_every_raster_is_one_coded_tile_whose_symbols_give_its_alpha(po, symbols):
    """A raster is its own normalize_rgba, one tile, coded by the oracle (its bytes depend on the alpha stream); the plain rule
    rebuilds its alpha plane from the oracle's alpha symbols; and the oracle's decode of its encode gives the raster."""
    ratio = []
    for name in A.names():
        r = A.raster(name)
        h, w, ch = r.shape
        assert ch == 4 and r[0, 0, 3] != 0 and (r[r[..., 3] == 0] == 0).all(), name
        assert np.array_equal(po.normalize_rgba(r), r), name
        assert len(po.tile_table(w, h, 4)) == 1, name
        blob = _blob(po, name)
        assert blob[3] >> 4 == 1 and len(blob) == int.from_bytes(blob[:3], "little"), (name, blob[3])
        ratio.append(len(blob) / r.size)
        a0, sy = symbols[name]
        assert np.array_equal(A.alpha_from_symbols(a0, sy, w, h), r[..., 3]), name
        assert np.array_equal(po.decode_tiles(1, blob, w, h, 4), r), name
    print("\n%d rasters, coded size %.0f %% .. %.0f %% of raw" % (len(ratio), 100 * min(ratio), 100 * max(ratio)))


def census(threads, symbols):
    """condition -> the rasters (or sizes) of the catalogue that meet it, for the walk of k_dec_resid<4, threads, true>"""
    PX = 4 * threads
    found = {}

    def note(cond, what):
        found.setdefault(cond, []).append(what)

    for (w, h) in A.SIZES:
        size, n = "%dx%d" % (w, h), w * h
        H = A.heads(w, h, threads)
        for hk in range(4):
            for key, sel in (("lane 0", H["lane"] == 0), ("lane 63", H["lane"] == 63), ("an interior lane", (H["lane"] > 0) & (H["lane"] < 63))):
                if (sel & (H["hk"] == hk)).any():
                    note("hk %d in %s" % (hk, key), size)
        if (H["tid"] == threads - 1).any():
            note("head in thread %d, the last of the workgroup" % (threads - 1), size)
        if (H["it"] == 0).any():
            note("head in iteration 0", size)
        if (H["it"] > 0).any():
            note("head in a later iteration", size)
        # per (iteration, wave): how many lanes begin inside the tile, how many of them hold a head
        wave_of = np.arange(0, n, 4) // 256                           # global wave index of every lane that begins inside the tile
        lanes = np.bincount(wave_of)
        with_head = np.bincount(np.unique(H["p"] // 4) // 64, minlength=len(lanes))
        if ((lanes == 64) & (with_head == 64)).any():
            note("a wave with a head in every lane", size)
        per_it = threads // 64
        for gw in np.flatnonzero(with_head == 0):
            first = gw // per_it * per_it
            if with_head[first:gw].any():                             # an earlier wave of the same iteration has one
                note("a wave without a head behind one that has one", size)
                break
        if n % 4:                                                     # the lane that holds the last pixels: columns w - n % 4 .. of the last row, so
            note("tile ends inside a lane, n mod 4 = %d" % (n % 4), size)   # its head would be pixel n itself and the tail test (i + hk < n) refuses it
        note("column-0 prologue of one iteration" if h - 1 <= threads else "column-0 prologue of several iterations", size)
        if n > PX:
            note("walk of several iterations", size)
        for name in A.of_size(w, h):
            a = A.raster(name)[..., 3]
            note("a hidden head" if (a[1:, 0] == 0).any() else "no hidden head", name)
            if (a[:, 0] != 0).all():
                note("only visible heads", name)
            D = A._deltas(symbols[name][1], w, h)
            if D[:, 0].sum() >= 256:
                note("column-0 sum passes 256", name)
            if (D[:, 1:].sum(axis=1) >= 256).any():
                note("a row sum passes 256", name)
    return found


NEEDED = (["hk %d in %s" % (hk, lane) for hk in range(4) for lane in ("lane 0", "lane 63", "an interior lane")] +
          ["head in iteration 0", "head in a later iteration", "a wave with a head in every lane", "a wave without a head behind one that has one",
           "a hidden head", "only visible heads", "tile ends inside a lane, n mod 4 = 1", "tile ends inside a lane, n mod 4 = 2",
           "tile ends inside a lane, n mod 4 = 3", "column-0 prologue of one iteration", "column-0 prologue of several iterations",
           "walk of several iterations", "column-0 sum passes 256", "a row sum passes 256"])


@pytest.mark.parametrize("threads", A.THREADS)
def test_census_the_catalogue_holds_every_named_condition(symbols, threads):
    """Printed with -s.  With w >= 4 no row start lies in the lane that straddles the tile's end: there the walk meets the opposite
    case, a head position (hk = n mod 4) that is pixel n itself, which `i + hk < t.n` must refuse."""
    found = census(threads, symbols)
    print("\n-- %d threads, %d pixels per iteration" % (threads, 4 * threads))
    for cond in sorted(found):
        print("  %-52s %3d  %s" % (cond, len(found[cond]), " ".join(found[cond][:6]) + (" .." if len(found[cond]) > 6 else "")))
    for cond in NEEDED + ["head in thread %d, the last of the workgroup" % (threads - 1)]:
        assert found.get(cond), (threads, cond)
    assert any(w > 4 * 64 * (threads // 256) for w, _ in A.SIZES)      # a width above 256 (above 1024 for the 1024-thread form)


def test_three_wrong_rules_give_other_planes(symbols):
    """Column 0 taken from the left neighbour in raster order differs on col0_*, sums that saturate on *_wrap and extremes, and a
    running sum that starts again at every 4 * threads pixels on every raster with such a pixel inside a row and a visible pixel in
    front of it: n > 4 * threads, except at widths 4 and 64, where every multiple of 1024 is a row start (a head sets the sum right
    whatever was carried), and except the four rasters listed at the end."""
    differ = {"col0": [], "saturated": [], 256: [], 1024: []}
    blind = []
    for name in A.names():
        kind, w, h = A.parse(name)
        a0, sy = symbols[name]
        right = A.alpha_from_symbols(a0, sy, w, h)
        if not np.array_equal(A.wrong_col0_from_left(a0, sy, w, h), right):
            differ["col0"].append(name)
        if not np.array_equal(A.wrong_saturated(a0, sy, w, h), right):
            differ["saturated"].append(name)
        for threads in A.THREADS:
            changed = not np.array_equal(A.wrong_restarted(a0, sy, w, h, threads), right)
            if changed:
                differ[threads].append(name)
            rs = A.restarts(w, h, threads)
            assert (len(rs) > 0) == (w * h > 4 * threads and (4 * threads) % w != 0), (name, threads)
            assert changed == bool(right.reshape(-1)[rs - 1].any()), (name, threads)   # it shows where a visible pixel stands in front
            if len(rs) and not changed:
                blind.append((name, threads))
    # 4095 = 5 * 819 = 7 * 585 = 63 * 65: in these four tiles of fewer than 8192 pixels the one pixel in front of 4096 is column 0, which
    # hidden_heads hides; the other kinds of the same sizes, and the same kind at 256 threads, show the rule
    assert blind == [("hidden_heads_%dx%d" % s, 1024) for s in ((5, 1031), (7, 599), (63, 70), (65, 67))], blind
    for key, got in differ.items():
        print("\n%s: differs on %d of %d" % (key, len(got), len(A.names())))
    for name in A.names():
        if fnmatch.fnmatch(name, "col0_*"):
            assert name in differ["col0"], name
        if fnmatch.fnmatch(name, "*_wrap_*") or name.startswith("extremes_"):
            assert name in differ["saturated"], name
    for threads in A.THREADS:                                        # (every kind is among them)
        assert {A.parse(nm)[0] for nm in differ[threads]} == set(A.KINDS), threads


# ================================================================================================ GPU: bytes against the oracle
def _report(name, got, threads):
    """what a failure says: the raster, its first wrong pixel, and where the walk of `threads` threads has that pixel and the head of its row"""
    r = A.raster(name)
    h, w, _ = r.shape
    bad = np.flatnonzero((got.reshape(h * w, 4) != r.reshape(h * w, 4)).any(axis=1))
    if not len(bad):
        return None
    p = int(bad[0])
    at, head = A.owner(p, w, threads)
    return ("%s: %d wrong pixels, the first %d (x %d, y %d): got %s, want %s; k_dec_resid<4, %d>: pixel in (iteration, wave, lane, k) %s, "
            "the head of its row in (iteration, wave, lane, hk) %s" % (name, len(bad), p, p % w, p // w, got.reshape(-1, 4)[p].tolist(),
                                                                        r.reshape(-1, 4)[p].tolist(), threads, at, head))


def _decode_host(blob, w, h, lib=None):
    """api.decode_tiles into a buffer with a guard behind it"""
    buf = np.full(w * h * 4 + GUARD, SENTINEL, np.uint8)
    api.decode_tiles(1, blob, w, h, 4, lib=lib, out=buf[: w * h * 4].reshape(h, w, 4))   # (raises on any status but 0)
    assert (buf[w * h * 4:] == SENTINEL).all(), "bytes behind the raster written"
    return buf[: w * h * 4].reshape(h, w, 4)


def _catalogue_through_the_host_call(po, threads, lib=None):
    for name in A.names():
        r = A.raster(name)
        got = _decode_host(_blob(po, name), r.shape[1], r.shape[0], lib)
        assert np.array_equal(got, r), _report(name, got, threads)


FORMS = [("XPNG_NARROW_RANS", 1024), ("XPNG_WIDE_RANS", 256)]
SAMPLE = ["rand_5x1031", "zeros_4x1100", "hidden_heads_1027x9", "extremes_65x67"]


@pytest.mark.gpu
@pytest.mark.parametrize("form,threads", FORMS)
def test_folded_form_on_every_raster(gpu, po, monkeypatch, tmp_path, form, threads):
    """k_dec_resid<4, 1024, true> (narrow chains) and, forced, k_dec_resid<4, 256, true> (wide chains): one image a call, so a tile
    is the whole launch.  A sample also goes through the files: xpng_store writes the oracle's bytes, xpng_load reads them back."""
    monkeypatch.setenv(form, "1")
    _catalogue_through_the_host_call(po, threads)
    for name in SAMPLE:
        r = A.raster(name)
        p = tmp_path / (name + ".xpng")
        gpu.store(1, r, str(p))
        assert p.read_bytes() == po.encode_image(1, r), name
        got = gpu.load(str(p))
        assert got.shape == r.shape and np.array_equal(got, r), _report(name, got, threads)


def _decode_pointers(decode, names, blobs):
    """decode(blob pointers, lengths, output pointers) of the oracle's blobs into guarded device buffers -> the buffers"""
    import torch
    d_o = [torch.full((A.raster(nm).size + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for nm in names]
    d_b = _upload(blobs)
    decode([t.data_ptr() for t in d_b], [len(b) for b in blobs], [t.data_ptr() for t in d_o])
    torch.cuda.synchronize()
    return d_o


def _compare(names, d_o, threads, what):
    for j, (nm, t) in enumerate(zip(names, d_o)):
        r, got = A.raster(nm), t.cpu().numpy()
        if not np.array_equal(got[: r.size].reshape(r.shape), r):
            pytest.fail("%s, image %d: %s" % (what, j, _report(nm, got[: r.size].reshape(r.shape), threads)))
        assert (got[r.size:] == SENTINEL).all(), (what, j, nm, "bytes behind the raster written")


@pytest.mark.gpu
def test_whole_catalogue_in_one_mixed_launch_takes_the_256_thread_fold(gpu, po):
    """Every raster in one MixedContext, the catalogue repeated until tiles x streams > 2048: the launch takes the wide chains and
    k_dec_resid<4, 256, true> by itself, as production does, with tiles of every geometry side by side in the 32-stream alpha
    groups.  Decoded twice on the one context."""
    names = A.mixed_names()
    blobs = [_blob(po, nm) for nm in names]
    ctx = gpu.MixedContext([(A.raster(nm).shape[1], A.raster(nm).shape[0]) for nm in names], 4)
    try:
        assert ctx.n_tiles == len(names) and ctx.n_tiles * A.SPT > 2048
        for turn in (1, 2):
            d_o = _decode_pointers(lambda b, n, o: ctx.decode_batch(1, b, n, o), names, blobs)
            assert ctx.decode_status() == 0, turn
            _compare(names, d_o, 256, "mixed launch, turn %d" % turn)
    finally:
        ctx.close()


B_WIDE = 2048 // A.SPT + 1                    # 205: the smallest batch with more than 2048 (tile, stream) items


@pytest.mark.gpu
@pytest.mark.parametrize("size", A.BATCH_SIZES)
def test_uniform_batch_of_one_geometry_takes_the_256_thread_fold(gpu, po, size):
    """Context(w, h, 4, batch=205) with the catalogue's planes of that geometry in turn: 32-stream alpha groups and workgroups of
    k_dec_resid<4, 256, true> that all walk the same geometry with different alpha."""
    assert (B_WIDE - 1) * A.SPT <= 2048 < B_WIDE * A.SPT
    of = A.of_size(*size)
    names = [of[j % len(of)] for j in range(B_WIDE)]
    blobs = [_blob(po, nm) for nm in names]
    ctx = gpu.Context(size[0], size[1], 4, batch=B_WIDE)
    try:
        assert ctx.n_tiles == 1
        d_o = _decode_pointers(lambda b, n, o: ctx.decode_device_batch(1, b, n, None, o), names, blobs)
        assert ctx.decode_status() == 0
        _compare(names, d_o, 256, "uniform batch %dx%d" % size)
    finally:
        ctx.close()


def _probes():
    if not os.path.exists(api.PROBES_SO):
        pytest.skip("the probes build of the library (make probes) is absent: XPNG_NO_ALPHA_FOLD exists only there")
    return api.probes_lib()


@pytest.mark.gpu
@pytest.mark.parametrize("form,threads", FORMS)
def test_plane_form_on_every_raster(gpu, po, monkeypatch, form, threads):
    """k_dec_alpha<1024> / <256> and k_dec_resid<4, ., false> on coded tiles of every geometry: the probes build with the fold
    switched off, loaded beside the release library."""
    P = _probes()
    assert api.hip_lib().xpnghip_probes_built() == 0 and P.xpnghip_probes_built() == 1
    monkeypatch.setenv("XPNG_NO_ALPHA_FOLD", "1")
    monkeypatch.setenv(form, "1")
    _catalogue_through_the_host_call(po, threads, lib=P)


# k_dec_parse has no rule about a tile's width, and decode_m1_plan answers a tile under 4 px with the plane form: the RELEASE library
# accepts a coded RGBA tile 1, 2 or 3 px wide.  The oracle's decoder (decode_tile_m1) has no rule about it either and keeps inside its
# buffers at any width (its symbol pool is sized by n).  No encoder writes such a tile, so these are crafted: one k word (a first pixel
# of 0x77 on every channel), every visible pixel in context 0 with a residual of no bits, and the alpha stream of a plane of ours.
NARROW = [(1, 1030), (2, 1030), (3, 1030)]    # more than 1024 rows: the column-0 prologue of both forms takes several iterations


def narrow_tile(po, w, h):
    """-> (blob, the oracle's decode of it).  Alpha: 1 .. 255 with every fifth pixel hidden and, at w = 3, a hidden column 0 on odd rows."""
    name = "narrow_%dx%d" % (w, h)
    a = np.where(A._noise(name, w, h, 4) % 5 == 0, 0, 1 + A._noise(name, w, h, 3) % 255)
    if w == 3:
        a[1::2, 0] = 0
    a[0, 0] = 0x77
    pa = np.empty_like(a)                     # the neighbour every alpha is predicted from: the left one, in column 0 the one above
    pa[:, 1:] = a[:, :-1]
    pa[1:, 0] = a[:-1, 0]
    sy = np.array([sym_of_delta(int(d)) for d in (a - pa).reshape(-1)[1:]], dtype=np.uint8)
    assert np.array_equal(A.alpha_from_symbols(0x77, sy, w, h), a.astype(np.uint8))
    visible = int((a.reshape(-1)[1:] != 0).sum())
    blob = tile_m1(0x10, [v2_blk1(visible, 0)] + [v2_blk0()] * 8 + [po.rans2_encode(np.bincount(sy, minlength=256), 256, sy, 15)])
    want = po.decode_tiles(1, blob, w, h, 4)
    assert np.array_equal(want[..., 3], a.astype(np.uint8)) and want[0, 0].tolist() == [0x77] * 4
    return blob, want


@pytest.mark.parametrize("w,h", NARROW)
def test_narrow_tiles_are_what_they_claim(po, w, h):
    """CPU: the crafted tile is one coded tile that the oracle decodes to the alpha plane it was built from, the colour 0x77 wherever
    a pixel and what it is predicted from are visible."""
    assert po.tile_table(w, h, 4) == [(0, 0, w, h)]
    blob, want = narrow_tile(po, w, h)
    assert blob[3] == 0x10 and len(blob) == int.from_bytes(blob[:3], "little") < 4 + 4 * w * h
    hidden = want[..., 3] == 0
    assert 0.1 < hidden.mean() < 0.6 and (want[hidden] == 0).all() and (want[~hidden][:, :3] == 0x77).any()


@pytest.mark.gpu
@pytest.mark.parametrize("form,threads", FORMS)
@pytest.mark.parametrize("w,h", NARROW)
def test_plane_form_in_the_release_library_on_tiles_under_4_px(gpu, po, monkeypatch, w, h, form, threads):
    """The only route to k_dec_alpha in the release library: rows of 1, 2 and 3 bytes that start at every byte alignment, and the
    early return at w = 1.  Expected pixels: the oracle's decode."""
    monkeypatch.setenv(form, "1")
    blob, want = narrow_tile(po, w, h)
    got = _decode_host(blob, w, h)
    bad = np.flatnonzero((got != want).any(axis=2).reshape(-1))
    assert not len(bad), (w, h, threads, len(bad), "first wrong pixel", int(bad[0]), got.reshape(-1, 4)[bad[0]].tolist(), want.reshape(-1, 4)[bad[0]].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("form", [f for f, _ in FORMS])
def test_encode_of_every_raster_is_the_oracles(gpu, po, monkeypatch, form):
    """The other direction, once: k_m1_transform_* predicts alpha from the pixel above in column 0, and the blobs the decode tests
    read are the ones the device writes."""
    monkeypatch.setenv(form, "1")
    for name in A.names():
        assert api.encode_tiles(1, A.raster(name)) == _blob(po, name), (name, form)
