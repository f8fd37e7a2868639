"""Calls in sequence on ONE context, different content every call (tests/_sequences.py), against the oracle.

A context keeps its workspace between calls.  The only clears in the core codec are d_sums (launch_chooser), d_flags2 / d_stream_n2 /
d_blk2 (level-2 encode), blk2 (level-2 decode) and d_status; everything else - stream lengths, k counts, block sizes, tile headers,
the WPrep records, staged words, the interleaved alpha tables, the top-class cut, the packed nibble queues, the arena that the
decode shares with the encode's stream scratch, the host-side nlh_generic - is right only because each launch overwrites what its
next reader takes.  The rest of the suite runs fresh contexts, or the same data twice; a data loader or an image server calls one
context with a different image every time, and that is what runs here.

The CPU part (not marked gpu) proves the orderings (every ordered pair of a family's rasters occurs exactly once) and the
transition census: over the consecutive calls of the sequences every context stream, the k words and the alpha block shrink and
grow, every block form follows every other, tiles change between raw, coded and coding nothing, every predictor follows every other,
and every level-2 tile kind follows every other.  The GPU part walks those sequences through encode_device[_batch],
decode_device[_batch], decode_region_batch and transform_device, at levels 1 and 2, in the narrow form, the wide form
(XPNG_WIDE_RANS=1) and alternating between them per call (the environment is read per call).  Every call is compared with the
oracle's bytes (encode_tiles) or with the raster (which the oracle's decode_tiles of those bytes gives: asserted once per raster),
never with an earlier GPU result, and the sentinel around every output is checked.  No timing and no tolerance anywhere."""
import numpy as np
import pytest

import _kit as K
import _sequences as Q
import _steered as S
from _kit import gpu, po

FORMS = ["narrow", "wide", "alternating"]
# chain -> (family, the level of call i is levels[i % len(levels)])
CHAINS = {"rgba_l1": ("rgba_l1", (1,)), "rgb_l1": ("rgb_l1", (1,)), "rgb_l2": ("rgb_l2", (2,)),
          "rgb_l1l2": ("rgb_l2", (1, 2)), "rgb_l2l1": ("rgb_l2", (2, 1))}


def form_at(form, i):
    return form if form != "alternating" else ("wide", "narrow")[i % 2]


# ================================================================================================ CPU: orderings and census
_ORACLE = {}


def _want(po, name, level):
    """What the oracle makes of a named raster at `level`: blobs, tile offsets (with the end behind them) and profile; its decode of
    the blobs is the raster.  Computed once, shared, never changed."""
    if (name, level) not in _ORACLE:
        r = Q.raster(name)
        h, w, ch = r.shape
        blobs = po.encode_tiles(level, r)
        assert np.array_equal(po.decode_tiles(level, blobs, w, h, ch), r), (name, level)
        prof = Q.profile(level, blobs, w, h, ch)
        _ORACLE[(name, level)] = {"blobs": blobs, "offs": [t["off"] for t in prof] + [len(blobs)], "prof": prof}
    return _ORACLE[(name, level)]


@pytest.mark.parametrize("k", [2, 3, 6, 7, 8])
def test_circuit_holds_every_ordered_pair_exactly_once(k):
    c = Q.circuit(k)
    assert len(c) == k * (k - 1) + 1 and c[0] == c[-1] == 0 and c == Q.circuit(k)
    pairs = list(zip(c, c[1:]))
    assert sorted(pairs) == [(a, b) for a in range(k) for b in range(k) if a != b]


def test_geometries(po):
    """One context serves a family: every raster of it has the main geometry.  The range geometries have tiles enough, and
    FORM_GEOM has tiles on both sides of TR_MAXW (a range of it selects the LDS-staged transform, another the generic one)."""
    assert [t[2] for t in po.tile_table(*Q.GEOM, 4)] == [456, 444]
    for fam in Q.FAMILIES.values():
        assert 6 <= len(fam) <= 8
        for name in fam:
            assert Q.raster(name).shape[:2] == Q.GEOM[::-1], name
    assert len(po.tile_table(*Q.RANGE_GEOM, 3)) == 4
    assert [t[2] for t in po.tile_table(*Q.FORM_GEOM, 4)] == [701, 601, 601] and 601 <= Q.TR_MAXW < 701
    for ch in (3, 4):
        for g in (Q.GEOM, Q.RANGE_GEOM, Q.FORM_GEOM, (64, 48)):
            assert S.tile_table(*g) == [tuple(int(v) for v in t) for t in po.tile_table(*g, ch)]


@pytest.mark.parametrize("family", list(Q.FAMILIES))
def test_census_of_transitions_between_consecutive_calls(po, family):
    """The acceptance census: what changes on some tile between consecutive calls of a family's sequence."""
    level = 2 if family == "rgb_l2" else 1
    seq = Q.sequence(family)
    seen = Q.transitions([(level, _want(po, n, level)["prof"]) for n in seq])
    print(family, len(seq), "calls:", sorted(seen, key=str))
    missing = Q.wanted(family) - seen
    assert not missing, missing
    for (fam, tr), why in Q.UNREACHABLE.items():
        if fam == family:
            assert tr not in seen, (tr, "listed as unreachable, but the sequence shows it:", why)
    if level == 2:                                                             # each predictor on a colour tile; every gray mode by its own tile
        profs = [t for n in Q.FAMILIES[family] for t in _want(po, n, 2)["prof"]]
        assert {t["pr"] for t in profs if t["kind"] == "colour"} == {0, 1, 2, 3}
        for n, kinds in Q.FAMILIES[family].items():
            got = [t["kind"] for t in _want(po, n, 2)["prof"]]
            assert got == ["colour" if k.startswith("pr") else k for k in kinds], (n, got)
    else:                                                                      # the tiles are what their names say
        for n, kinds in Q.FAMILIES[family].items():
            for k, t in zip(kinds, _want(po, n, 1)["prof"]):
                assert t["kind"] == {"raw": "raw", "clear": "nothing"}.get(k, "coded"), (n, k, t["kind"])
                if k.startswith("pr"):
                    assert t["pr"] == int(k[2:]) and all(f == "coded" for f in t["forms"][:4]) and min(t["ctx_n"]) > 0, (n, k)
        if family == "rgba_l1":                                                # the last coded pixel lies further up, inside a row
            a = Q.raster("a_tail_tail")[..., 3]
            assert (a[-1] == 0).all() and (a[2 * Q.GEOM[1] // 3 - 1, :200] != 0).any() and a[2 * Q.GEOM[1] // 3 - 1, -1] == 0


def test_the_alternating_level_chain_changes_level_on_every_call(po):
    """rgb_l1l2 / rgb_l2l1 walk the level-2 family with the level alternating: between them every ordered pair of rasters occurs
    with either order of the two levels."""
    seq = Q.sequence("rgb_l2")
    seen = set()
    for chain in ("rgb_l1l2", "rgb_l2l1"):
        levels = CHAINS[chain][1]
        for i in range(1, len(seq)):
            seen.add((seq[i - 1], levels[(i - 1) % 2], seq[i], levels[i % 2]))
    names = list(Q.RGB_L2)
    assert seen == {(a, la, b, 3 - la) for a in names for b in names if a != b for la in (1, 2)}


def test_rasters_of_the_other_geometries_differ_from_call_to_call(po):
    """The tile-range and region rasters carry one predictor each on every tile, so consecutive calls change it everywhere;
    the 64 x 48 pool of the production pairing holds the four predictors, a raw tile, a tile that codes nothing and every block form."""
    for name in Q.WIDE:
        levels = (1,) if name.startswith("a_") else (1, 2)
        for level in levels:
            assert {t.get("pr") for t in _want(po, name, level)["prof"]} == {int(name[4])}, (name, level)
    profs = [_want(po, n, 1)["prof"][0] for n in Q.SMALL]
    assert len(po.tile_table(64, 48, 4)) == 1 and {t["kind"] for t in profs} == {"raw", "nothing", "coded"}
    assert {t["pr"] for t in profs if t["kind"] == "coded"} == {0, 1, 2, 3}
    assert {f for t in profs if "forms" in t for f in t["forms"]} == set(Q.BLOCK_FORMS)


# ================================================================================================ GPU: one context, call after call
_DEV = {}


def _dev_raster(name):
    import torch
    if ("r", name) not in _DEV:
        _DEV[("r", name)] = torch.from_numpy(np.concatenate([Q.raster(name).reshape(-1), np.zeros(64, np.uint8)])).cuda()
    return _DEV[("r", name)]


def _dev_blobs(po, name, level):
    if ("b", name, level) not in _DEV:
        _DEV[("b", name, level)] = K._upload([_want(po, name, level)["blobs"]])[0]
    return _DEV[("b", name, level)]


def first_stage_that_differs(ctx, po, raster, ti, level):
    """After an encode of `raster` (image 0 of the call): the first stage of tile `ti` whose fetched state is not the oracle's -
    sums, predictor, planes, streams, k, blocks - or None.  (Level 2 leaves only the chooser's stages to fetch.)"""
    h, w, ch = raster.shape
    t = po.tile_table(w, h, ch)[ti]
    pr, sums = po.choose_predictor(raster, t)
    if ctx.fetch("sums", ti).view(np.uint32).tolist() != sums:
        return "sums"
    if int(ctx.fetch("pr", ti)[0]) != pr:
        return "predictor"
    if level != 1:
        return None
    planes = po.m1_planes(raster, t, pr)
    for k in ("nl", "r", "g", "b"):
        if not np.array_equal(ctx.fetch(k, ti), planes[k]):
            return f"planes ({k})"
    if ch == 4 and not np.array_equal(ctx.fetch("a", ti)[1:], planes["a"][1:]):     # (the first bytes hold column 0's alphas by now)
        return "planes (a)"
    st = po.m1_streams(raster, t, planes)
    for c in range(9):
        if not np.array_equal(ctx.fetch(10 + c, ti), st["ctx"][c]):
            return f"streams (context {c})"
    if not np.array_equal(ctx.fetch("k", ti).view(np.uint32), st["k"]):
        return "k"
    for c in range(9):
        if ctx.fetch(20 + c, ti).tobytes() != po.rans2_encode(st["F"][c], 9, st["ctx"][c], 12):
            return f"blocks (context {c})"
    if ch == 4 and ctx.fetch(29, ti).tobytes() != po.rans2_encode(st["FA"], 256, planes["a"][1:], 15):
        return "blocks (alpha)"
    return None


class Run:
    """One context and the calls made on it so far.  Every call refills its output arena with the sentinel first, so nothing an
    earlier call wrote can pass for this call's output."""

    def __init__(self, gpu, po, monkeypatch, w, h, ch, batch=1):
        self.po, self.mp, self.w, self.h, self.ch, self.B = po, monkeypatch, w, h, ch, batch
        self.ctx = gpu.Context(w, h, ch, batch=batch)
        assert self.ctx.tiles() == po.tile_table(w, h, ch)
        self.enc = K.Arena([self.ctx.blob_bound()] * batch, es=16)
        self.dec = K.Arena([w * h * ch] * batch, es=16)
        self.i, self.prev, self.cur = 0, "none (a fresh context)", None

    def close(self):
        self.ctx.close()

    def _begin(self, op, names, level, form, **more):
        self.cur = f"{op} {'+'.join(names)} level {level} {form}" + "".join(f" {k}={v}" for k, v in more.items())
        if form == "wide":
            self.mp.setenv("XPNG_WIDE_RANS", "1")
        else:
            self.mp.delenv("XPNG_WIDE_RANS", raising=False)

    def _end(self):
        self.prev, self.i = self.cur, self.i + 1

    def fail(self, what):
        return f"call {self.i}: {self.cur}: {what}; previous call: {self.prev}"

    def _fetch(self, arena, sizes):
        try:
            return arena.fetch(sizes + [0] * (self.B - len(sizes)))
        except AssertionError as e:
            raise AssertionError(self.fail(str(e))) from None

    def encode(self, names, level, form, t0=0, t1=None):
        """names: one raster per image of the call.  A range call's bytes are that piece of the oracle's."""
        t1 = self.ctx.n_tiles if t1 is None else t1
        self._begin("encode", names, level, form, tiles=(t0, t1))
        wants = []
        for n in names:
            e = _want(self.po, n, level)
            wants.append(e["blobs"][e["offs"][t0]:e["offs"][t1]])
        self.enc.refill()
        rp = [_dev_raster(n).data_ptr() for n in names]
        if self.B == 1:
            lens = [self.ctx.encode_device(level, rp[0], self.enc.ptrs[0], t0=t0, t1=t1)]
        else:
            lens = self.ctx.encode_device_batch(level, rp, self.enc.ptrs[:len(names)], t0=t0, t1=t1)
        got = self._fetch(self.enc, [min(n, self.enc.sizes[0]) for n in lens])
        for j, (n, want) in enumerate(zip(names, wants)):
            g = got[j].tobytes()
            if g == want:
                continue
            m = min(len(g), len(want))
            at = next((x for x in range(m) if g[x] != want[x]), m)
            offs = _want(self.po, n, level)["offs"]
            ti = max(t for t in range(t0, t1) if offs[t] - offs[t0] <= at)
            stage = first_stage_that_differs(self.ctx, self.po, Q.raster(n), ti, level) if j == 0 else "not fetched (image 0 only)"
            raise AssertionError(self.fail(f"image {j} ({n}): {len(g)} bytes for {len(want)}, the first that differs is byte {at}, in "
                                           f"tile {ti}; first stage that differs: {stage}"))
        self._end()

    def decode(self, names, level, form, offs):
        """offs: 'host' (the caller gives the tile offsets) or 'walk' (tile_offs=None: the size walk runs on the device)"""
        self._begin("decode", names, level, form, offsets=offs)
        es = [_want(self.po, n, level) for n in names]
        self.dec.refill()
        bp = [_dev_blobs(self.po, n, level).data_ptr() for n in names]
        lens = [len(e["blobs"]) for e in es]
        to = [e["offs"][:-1] for e in es] if offs == "host" else None
        if self.B == 1:
            self.ctx.decode_device(level, bp[0], lens[0], to[0] if to else None, self.dec.ptrs[0])
        else:
            self.ctx.decode_device_batch(level, bp, lens, to, self.dec.ptrs[:len(names)])
        status = self.ctx.decode_status()
        assert status == 0, self.fail(f"decode_status() = {status}")
        got = self._fetch(self.dec, [self.w * self.h * self.ch] * len(names))
        for j, n in enumerate(names):
            self._same_pixels(got[j].reshape(self.h, self.w, self.ch), Q.raster(n), 0, 0, f"image {j} ({n})")
        self._end()

    def _same_pixels(self, got, want, x0, y0, what):
        if np.array_equal(got, want):
            return
        ys, xs = np.nonzero((got != want).any(axis=2))
        x, y = int(xs[0]) + x0, int(ys[0]) + y0
        ti = next(i for i, (tx, ty, tw, th) in enumerate(self.ctx.tiles()) if tx <= x < tx + tw and ty <= y < ty + th)
        raise AssertionError(self.fail(f"{what}: {len(ys)} pixels differ, the first at ({x}, {y}), in tile {ti}"))

    def region(self, names, level, form, rects):
        """decode_region_batch: image j's rects[j] = (x, y, w, h) at one row pitch with room behind every row, which stays untouched"""
        self._begin("region", names, level, form, rects=rects)
        es = [_want(self.po, n, level) for n in names]
        bpr = max(r[2] for r in rects) * self.ch + 64
        out = K.Arena([r[3] * bpr for r in rects], es=16)
        self.ctx.decode_region_batch(level, [_dev_blobs(self.po, n, level).data_ptr() for n in names], [len(e["blobs"]) for e in es],
                                     rects, out.ptrs, bpr)
        status = self.ctx.decode_status()
        assert status == 0, self.fail(f"decode_status() = {status}")
        try:
            got = out.fetch()
        except AssertionError as e:
            raise AssertionError(self.fail(str(e))) from None
        for j, (n, (x, y, w, h)) in enumerate(zip(names, rects)):
            rows = got[j].reshape(h, bpr)
            assert (rows[:, w * self.ch:] == K.SENTINEL).all(), self.fail(f"image {j} ({n}): bytes behind a row were written")
            self._same_pixels(rows[:, : w * self.ch].reshape(h, w, self.ch), Q.raster(n)[y:y + h, x:x + w], x, y, f"image {j} ({n})")
        self._end()

    def transform(self, name, form):
        self._begin("transform", [name], 1, form)
        self.ctx.transform_device(_dev_raster(name).data_ptr())
        r = Q.raster(name)
        for ti, t in enumerate(self.ctx.tiles()):
            pr, sums = self.po.choose_predictor(r, t)
            assert self.ctx.fetch("sums", ti).view(np.uint32).tolist() == sums, self.fail(f"tile {ti}: sums")
            planes = self.po.m1_planes(r, t, pr)
            for k in ("nl", "r", "g", "b") + (("a",) if self.ch == 4 else ()):
                assert np.array_equal(self.ctx.fetch(k, ti), planes[k]), self.fail(f"tile {ti}: plane {k}")
        self._end()


def _chain(name):
    fam, levels = CHAINS[name]
    seq = Q.sequence(fam)
    ch = Q.raster(seq[0]).shape[2]
    return seq, levels, ch


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("chain", list(CHAINS))
def test_encode_chain(gpu, po, monkeypatch, chain, form):
    """encode_device along the circuit of a family: every ordered pair (previous raster, this raster) once, so every transition of
    the census once.  A stale chooser sum, stream length, k count, block size, tile header or table from the previous call gives
    other bytes, and the message names the stage where it entered."""
    seq, levels, ch = _chain(chain)
    run = Run(gpu, po, monkeypatch, *Q.GEOM, ch)
    try:
        for i, name in enumerate(seq):
            run.encode([name], levels[i % len(levels)], form_at(form, i))
    finally:
        run.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("offs", ["host", "walk", "alternating"])
@pytest.mark.parametrize("chain", list(CHAINS))
def test_decode_chain(gpu, po, monkeypatch, chain, offs, form):
    """decode_device over the oracle's blobs along the circuit, with host-given tile offsets, with the device size walk, and
    alternating between the two (in pairs of calls, so that the alternation does not follow the form's or the level's)."""
    seq, levels, ch = _chain(chain)
    run = Run(gpu, po, monkeypatch, *Q.GEOM, ch)
    try:
        for i, name in enumerate(seq):
            run.decode([name], levels[i % len(levels)], form_at(form, i), offs if offs != "alternating" else ("host", "walk")[(i // 2) % 2])
    finally:
        run.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("first", ["encode", "decode"])
@pytest.mark.parametrize("chain", list(CHAINS))
def test_encode_and_decode_take_turns(gpu, po, monkeypatch, chain, first, form):
    """The circuit walked with encode on even calls and decode on odd calls, then with the parities swapped: the decode's arena is
    the encode's stream scratch, and each direction leaves its lengths, tables and headers where the other's stand."""
    seq, levels, ch = _chain(chain)
    run = Run(gpu, po, monkeypatch, *Q.GEOM, ch)
    try:
        for i, name in enumerate(seq):
            if (i % 2 == 0) == (first == "encode"):
                run.encode([name], levels[i % len(levels)], form_at(form, i))
            else:
                run.decode([name], levels[i % len(levels)], form_at(form, i), ("host", "walk")[(i // 2) % 2])
    finally:
        run.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("chain", ["rgba_l1", "rgb_l1", "rgb_l2"])
def test_batch_slots(gpu, po, monkeypatch, chain, form):
    """Context(batch=3): calls with 3, 1, 2, 3, 2, 1, 3 images, an encode and a decode each, the rasters moved on by one slot per
    call.  Every image is checked, and so is the sentinel around every output - the unused slots' outputs included."""
    fam, levels = CHAINS[chain]
    names = list(Q.FAMILIES[fam])
    run = Run(gpu, po, monkeypatch, *Q.GEOM, Q.raster(names[0]).shape[2], batch=3)
    try:
        for i, k in enumerate((3, 1, 2, 3, 2, 1, 3)):
            pick = [names[(i + j) % len(names)] for j in range(k)]
            run.encode(pick, levels[0], form_at(form, i))
            run.decode(pick[::-1], levels[0], form_at(form, i), ("host", "walk")[i % 2])
    finally:
        run.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("fmt,level,geom", [("a", 1, Q.RANGE_GEOM), ("b", 1, Q.RANGE_GEOM), ("b", 2, Q.RANGE_GEOM), ("a", 1, Q.FORM_GEOM), ("b", 1, Q.FORM_GEOM)],
                         ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))
def test_tile_ranges(gpu, po, monkeypatch, fmt, level, geom, form):
    """whole -> [1, 2) -> [0, 1) -> whole -> [1, N) -> [0, 1) -> whole, a raster with another predictor each call (the per-range
    d_sums clears, order_for).  1903 x 328 has tiles on both sides of TR_MAXW = 672 (701 / 601 / 601 columns): there the calls
    switch the transform between the generic kernel (a range with tile 0) and the LDS-staged one (a range without it), and with it
    the form of the nl histogram records that the host-side nlh_generic describes."""
    w, h = geom
    run = Run(gpu, po, monkeypatch, w, h, 4 if fmt == "a" else 3)
    N = run.ctx.n_tiles
    try:
        for i, (t0, t1) in enumerate(((0, N), (1, 2), (0, 1), (0, N), (1, N), (0, 1), (0, N))):
            run.encode([f"{fmt}_pr{(i + level) % 4}_{w}x{h}"], level, form_at(form, i), t0, t1)
    finally:
        run.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("fmt,level", [("a", 1), ("b", 1), ("b", 2)])
def test_region_then_whole(gpu, po, monkeypatch, fmt, level, form):
    """1000 x 900, four tiles: a region inside tile 0 of A, a full decode of B, a region of C over all four tiles, a region of D
    inside tile 3, a full decode of A."""
    w, h = Q.RANGE_GEOM
    run = Run(gpu, po, monkeypatch, w, h, 4 if fmt == "a" else 3)
    A, B, C, D = (f"{fmt}_pr{p}_{w}x{h}" for p in range(4))
    try:
        run.region([A], level, form_at(form, 0), [(10, 20, 300, 200)])
        run.decode([B], level, form_at(form, 1), "walk")
        run.region([C], level, form_at(form, 2), [(500, 400, 450, 480)])
        run.region([D], level, form_at(form, 3), [(600, 500, 300, 300)])
        run.decode([A], level, form_at(form, 4), "host")
    finally:
        run.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("family", ["rgba_l1", "rgb_l1"])
def test_stage_entry_then_encode(gpu, po, monkeypatch, family, form):
    """transform_device on A, then encode_device on B: sums, predictor, the planes, the nine streams, k and the blocks of B are the
    oracle's, on both tiles, for the first pairs of the circuit."""
    seq = Q.sequence(family)[:9]
    run = Run(gpu, po, monkeypatch, *Q.GEOM, Q.raster(seq[0]).shape[2])
    try:
        for i in range(0, 8, 2):
            run.transform(seq[i], form_at(form, i))
            run.encode([seq[i + 1]], 1, form_at(form, i + 1))
            for ti in range(run.ctx.n_tiles):
                stage = first_stage_that_differs(run.ctx, po, Q.raster(seq[i + 1]), ti, 1)
                assert stage is None, f"after call {run.i - 1} ({run.prev}; before it transform {seq[i]}): tile {ti}: {stage}"
    finally:
        run.close()


@pytest.mark.gpu
def test_production_pairing(gpu, po, monkeypatch):
    """230 single-tile RGBA rasters of 64 x 48 in one batch: 2300 (tile, stream) items select the wide chains and the 256-thread
    routing by themselves.  Three encode and three decode calls take turns, the contents moved on by one slot per call."""
    names = list(Q.SMALL)
    B = 230
    run = Run(gpu, po, monkeypatch, 64, 48, 4, batch=B)
    assert run.ctx.n_tiles * 10 * B > 2048
    try:
        for i in range(3):
            run.encode([names[(i + j) % len(names)] for j in range(B)], 1, "by size")
            run.decode([names[(2 * i + 3 * j) % len(names)] for j in range(B)], 1, "by size", ("walk", "host")[i % 2])
    finally:
        run.close()
