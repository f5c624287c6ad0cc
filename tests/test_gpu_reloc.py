"""Relocalisation on the GPU: the frame code, the batched
keyframe search, the store, kfx_relocalise and kfx_pipeline_recover.  Every
comparison is exact: codes as words, matches entry for entry in match order,
results field by field with poses as bits.  The reference is reloc_cases (numpy
and Python integers); tests/test_reloc_cases.py asserts what the retrieval
family has to contain."""
import ctypes as C
import functools

import numpy as np
import pytest

import kfx
import multi_cases as M
import oracle as O
import reloc_cases as R
import view_cases as VC
from kfx import KFX_FRAME_CUR, KFX_FRAME_PREV, KFX_OK, KFX_TRACKING_LOST, Keyframes, KinectFusion, synth
from kfx.abi import FERN_DTYPE, Intrinsics, KeyframeMatch, Pose, RecoverParams, RelocResult, default_params

pytestmark = pytest.mark.gpu
f32 = np.float32


def small_ctx(w, h, L):
    p = default_params(dims=64, range_m=2.048)
    p.pyramid_height = L
    return KinectFusion(Intrinsics(w, h, 0.8 * w, 0.8 * w, (w - 1) / 2.0, (h - 1) / 2.0), p)


def coarse(kf):
    return kf.frame_maps(KFX_FRAME_CUR, kf.params.pyramid_height - 1)[0]


def words(a):
    return np.asarray(a, np.uint64).tolist()


@functools.lru_cache(maxsize=None)
def frames8():
    intr = synth.Intrinsics.qvga()
    bgr, dep, _ = synth.sequence(8, intr, noise=True, dropout=0.01)
    return intr, bgr, dep.astype(f32)


# ---- 1. encode ----------------------------------------------------------------

@pytest.mark.parametrize("w,h,L", [(64, 48, 3), (32, 32, 1)])
def test_encode_crafted(w, h, L):
    """Ferns at the grid's corners and along its last row and column; blocks whose sums equal the threshold
    (bit 0) or pass it by one (bit 1), per channel; td at the depth (0), one float below it (1), over a hole (0)."""
    wL, hL, s = R.grid(w, h, L)
    kf = small_ctx(w, h, L)
    try:
        pos = [(0, 0), (wL - 1, 0), (0, hL - 1), (wL - 1, hL - 1)]
        pos += [(x, hL - 1) for x in range(1, 7)] + [(wL - 1, y) for y in range(1, 7)]
        assert len(pos) == 16 and len(set(pos)) == 16
        depth = np.full((h, w), 1000.0, f32) + np.arange(w, dtype=f32)[None, :]
        depth[h // 2:, w // 2:] = 0.0  # a hole over the bottom-right quarter
        tab = np.zeros(16, FERN_DTYPE)
        for f, (x, y) in enumerate(pos):
            tab[f] = (x, y, 10 + f, 100 + f, 239 + f, 0, 0.0)
        base = np.zeros((h, w, 3), np.uint8)
        for f, (x, y) in enumerate(pos):
            base[y * s:(y + 1) * s, x * s:(x + 1) * s] = (tab[f]["tb"], tab[f]["tg"], tab[f]["tr"])
        kf.stage_preprocess(base, depth)
        d = coarse(kf)
        dv = np.array([d[y, x] for x, y in pos], f32)
        assert dv[3] == 0.0 and dv[0] > 0.9 and dv[1] > 0.9  # the hole and the surface, as the device filtered them
        td = dv.copy()
        td[1] = np.nextafter(dv[1], f32(-np.inf))  # one float below the depth: bit 3 set
        td[3] = 0.0                                # a hole against a zero threshold: 0 > 0 is false
        td[4:] = np.where(dv[4:] > 0, dv[4:], f32(0.5))
        tab["td"] = td
        with_tab = Keyframes(kf, table=tab)
        assert with_tab.m == 16 and with_tab.table().tobytes() == tab.tobytes()
        for chan in (None, 0, 1, 2):
            img = base.copy()
            if chan is not None:  # one pixel of every block one step brighter in that channel: sum = t s^2 + 1
                for x, y in pos:
                    img[y * s + s - 1, x * s + s - 1, chan] += 1
            kf.stage_preprocess(img, depth)
            assert np.array_equal(coarse(kf).view(np.uint32), d.view(np.uint32))
            nib = R.unpack(with_tab.encode())
            want = np.full(16, 0 if chan is None else 1 << chan, np.uint8)
            want[1] |= 8
            assert nib.tolist() == want.tolist(), chan
            assert words(with_tab.encode()) == words(R.encode(img, d, tab, s))
        with_tab.close()
    finally:
        kf.close()


@pytest.mark.parametrize("overlap", [False, True])
def test_encode_scene_frames(overlap):
    """The scene's QVGA frames at four table sizes: after kfx_pipeline, after kfx_stage_preprocess alone and
    after a staged frame, the code is the restated code of the downloaded dmap and the given image."""
    intr, bgr, dep = VC.scene()
    kf = KinectFusion(Intrinsics.from_any(intr), VC.params(64))
    kf.set_frame_overlap(overlap)
    stores = [Keyframes(kf, m=m) for m in (16, 48, 512, 1024)]
    try:
        for st in stores:
            assert st.table().tobytes() == R.table(320, 240, 3, m=st.m).tobytes()
        for k in range(VC.N_FRAMES):
            assert kf.pipeline(bgr[k], dep[k]) == KFX_OK
            d = coarse(kf)
            for st in stores:
                assert words(st.encode()) == words(R.encode(bgr[k], d, st.table(), 4)), (k, st.m)
            j = (k + 2) % VC.N_FRAMES
            kf.stage_preprocess(bgr[j], dep[j])
            d = coarse(kf)
            for st in stores:
                assert words(st.encode()) == words(R.encode(bgr[j], d, st.table(), 4)), (k, j, st.m)
        assert kf.keyframe_ms()["encode"] > 0.0
        kf.reset()
        kf.stage_frames(bgr, dep)
        assert kf.synchronize() == KFX_OK
        for k in range(VC.N_FRAMES):
            kf.pipeline_staged(k)  # no explicit sync before the encode
            code = stores[2].encode()
            assert words(code) == words(R.encode(bgr[k], coarse(kf), stores[2].table(), 4)), k
        assert kf.synchronize() == KFX_OK
    finally:
        for st in stores:
            st.close()
        kf.close()


# ---- 2. search ----------------------------------------------------------------

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 4100]


def brute(qn, cn, k):
    """reloc_cases.search on nibble arrays (q, m) and (n, m)."""
    out = np.full((len(qn), k, 2), -1, np.int32)
    if len(cn) == 0:
        return out
    for i in range(len(qn)):
        d = (cn != qn[i][None, :]).sum(axis=1).astype(np.int64)
        order = np.lexsort((np.arange(len(d)), d))[:k]
        out[i, :len(order), 0] = order
        out[i, :len(order), 1] = d[order]
    return out


@functools.lru_cache(maxsize=None)
def search_family(m):
    """4100 keyframe codes and 300 queries as nibbles: random with a fixed seed, plus crafted neighbours of
    query 0: one bit of a nibble for each of the four bits, all four bits of a nibble (distance still 1),
    every nibble (distance m), and equal codes on either side of a wave, a block and a grid boundary."""
    rng = np.random.default_rng(20251021 + m)
    cn = rng.integers(0, 16, (4100, m)).astype(np.uint8)
    qn = rng.integers(0, 16, (300, m)).astype(np.uint8)
    qn[1::3] = cn[rng.integers(0, 4100, len(qn[1::3]))]  # queries near a stored code
    qn[1::3, :3] ^= 1
    for bit in range(4):
        cn[1 + bit] = qn[0]
        cn[1 + bit, (5 * bit + 2) % m] ^= 1 << bit
    cn[5] = qn[0]
    cn[5, m - 1] ^= 15
    cn[6] = qn[0] ^ 15
    twin = qn[0].copy()
    twin[0] ^= 3
    twin[m // 2] ^= 8
    for i in (63, 64, 255, 256, 4095, 4096):
        cn[i] = twin
    return cn, qn


@pytest.mark.parametrize("m", [16, 512, 1024])
def test_search(m):
    """A store grown by single puts through every size, searched at each: brute force, entry for entry; the
    reversed batch reversed; and one store built at once gives the same answers."""
    cn, qn = search_family(m)
    codes = np.stack([R.pack(c) for c in cn])
    queries = np.stack([R.pack(c) for c in qn])
    assert np.array_equal(R.distances(queries[:2], codes[:8]), (cn[None, :8] != qn[:2, None]).sum(axis=2))
    assert R.search(queries[:3], codes[:70], 4).tolist() == brute(qn[:3], cn[:70], 4).tolist()
    kf = small_ctx(32, 32, 1)
    grown = Keyframes(kf, m=m)
    eye = Pose.identity()
    answers = {}
    try:
        for N in SIZES:
            while len(grown) < N:
                assert grown.put(eye, codes[len(grown)]) == len(grown) - 1
            for k in (1, 4, 16):
                for q in (1, 3, 17):
                    got = grown.search(queries[:q], k)
                    assert got.tolist() == brute(qn[:q], cn[:N], k).tolist(), (N, k, q)
                    answers[(N, k, q)] = got
            got = grown.search(queries[:17][::-1], 4)
            assert got.tolist() == answers[(N, 4, 17)][::-1].tolist(), N
        if m == 512:  # the crafted neighbours of query 0, by hand
            top = answers[(4100, 16, 1)][0].tolist()
            assert top[:11] == [[1, 1], [2, 1], [3, 1], [4, 1], [5, 1], [63, 2], [64, 2], [255, 2], [256, 2],
                                [4095, 2], [4096, 2]]
            d6 = int((cn[6] != qn[0]).sum())
            assert d6 == m
        # a batch that crosses the chunk rule's boundaries: 9 queries to a block, the last block 3
        assert kfx.keyframes_search_chunk(4100, 300) == 9
        got = grown.search(queries, 4)
        assert got.tolist() == brute(qn, cn, 4).tolist()
        assert kf.keyframe_ms()["search"] > 0.0
        once = Keyframes(kf, m=m)
        for c in codes:
            once.put(eye, c)
        for (N, k, q), want in answers.items():
            if N == 4100:
                assert once.search(queries[:q], k).tolist() == want.tolist(), (k, q)
        assert once.search(queries, 4).tolist() == got.tolist()
        once.close()
    finally:
        grown.close()
        kf.close()


def test_search_equal_codes_and_edges():
    """Every distance 0: the ids decide.  q = 0, argument errors write nothing."""
    kf = small_ctx(32, 32, 1)
    st = Keyframes(kf, m=48)
    L = kfx.lib()
    try:
        code = R.pack(np.arange(48) % 16)
        for _ in range(300):
            st.put(Pose.identity(), code)
        got = st.search([code, code], 16)
        assert got[..., 0].tolist() == [list(range(16))] * 2 and not got[..., 1].any()
        far = R.pack((np.arange(48) + 1) % 16)
        assert st.search([far], 2).tolist() == [[[0, 48], [1, 48]]]
        out = np.full((4, 2), -9, np.int32)
        cp = code.ctypes.data_as(C.POINTER(C.c_uint64))
        assert L.kfx_keyframes_search(kf._h, st._h, cp, 0, 4, out.ctypes.data) == 0
        for q, k in ((-1, 4), (65537, 4), (1, 0), (1, 17)):
            assert L.kfx_keyframes_search(kf._h, st._h, cp, q, k, out.ctypes.data) == -1
        assert L.kfx_keyframes_search(kf._h, st._h, cp, 1, 4, None) == -1
        assert L.kfx_keyframes_search(kf._h, None, cp, 1, 4, out.ctypes.data) == -1
        assert np.all(out == -9)
        other = small_ctx(64, 48, 3)  # a store of another grid
        assert L.kfx_keyframes_search(other._h, st._h, cp, 1, 4, out.ctypes.data) == -1
        assert L.kfx_encode_frame(other._h, st._h, cp) == -1 and np.all(out == -9)
        other.close()
    finally:
        st.close()
        kf.close()


# ---- 3. the store -------------------------------------------------------------

def test_store_get_export_import_consider():
    F = R.family(4)
    intr = synth.Intrinsics.qvga()
    kf = KinectFusion(Intrinsics.from_any(intr), R.params())
    st = Keyframes(kf)
    try:
        assert st.m == 512 and st.table().tobytes() == F["table"].tobytes()
        # kfx_keyframes_consider on key 0, its revisit, key 1, its revisit, ...: the restated harvest
        feed = [fr for pair in zip(F["key"], F["revisit"]) for fr in pair]
        held = []
        for i, (bgr, dep, dmap, code) in enumerate(feed):
            kf.stage_preprocess(bgr, dep)
            assert np.array_equal(coarse(kf).view(np.uint32), dmap.view(np.uint32))  # the oracle's map
            assert words(st.encode()) == words(code)
            near = R.search([code], held, 1)[0, 0].tolist()
            want = len(held) if not held or near[1] > R.HARVEST_MIN_DISTANCE else -1
            got, nearest = st.consider(R.HARVEST_MIN_DISTANCE)
            assert (got, list(nearest)) == (want, near), i
            if want >= 0:
                held.append(code)
        assert len(st) == len(held) == 4
        pose = M.twist_matrix((0.1, -0.2, 0.05), (0.3, -0.1, 0.7))
        kid = st.put(pose, F["query"][0][3])
        kf.stage_preprocess(*F["query"][1][:2])
        kid2 = st.add(pose)
        assert (kid, kid2) == (4, 5)
        for k, code in ((kid, F["query"][0][3]), (kid2, F["query"][1][3]), (1, held[1])):
            P, c = st.get(k)
            assert words(c) == words(code)
            assert bytes(P) == (bytes(Pose.from_matrix(pose)) if k >= 4 else bytes(Pose.identity()))
        assert kfx.lib().kfx_keyframes_get(st._h, 6, None, None) == -1
        queries = np.stack([q[3] for q in F["query"]] + held)
        want = R.search(queries, held + [F["query"][0][3], F["query"][1][3]], 4)
        assert st.search(queries, 4).tolist() == want.tolist()
        assert st.search(None, 3).tolist() == R.search([F["query"][1][3]], held + [F["query"][0][3],
                                                                                   F["query"][1][3]], 3).tolist()
        # the blob: parsed by the restatement, imported into a fresh context, refused by another grid
        blob = st.export()
        B = R.blob_parse(blob)
        assert (B["m"], B["wL"], B["hL"], B["s"], B["seed"], B["depth_mm"]) == (512, 80, 60, 4, 2013, (400, 4000))
        assert B["table"].tobytes() == F["table"].tobytes() and len(B["codes"]) == 6
        fresh = KinectFusion(Intrinsics.from_any(intr), R.params())
        back = Keyframes.load(fresh, blob)
        assert len(back) == 6 and back.search(queries, 4).tolist() == want.tolist()
        for k in range(6):
            (Pa, ca), (Pb, cb) = st.get(k), back.get(k)
            assert bytes(Pa) == bytes(Pb) and words(ca) == words(cb)
        assert back.export() == blob
        back.close()
        fresh.close()
        other = small_ctx(64, 48, 3)
        h = C.c_void_p()
        b = np.frombuffer(blob, np.uint8)
        L = kfx.lib()
        assert L.kfx_keyframes_import(other._h, b.ctypes.data, b.size, C.byref(h)) == -1 and not h.value
        assert L.kfx_keyframes_import(kf._h, b.ctypes.data, b.size - 1, C.byref(h)) == -1 and not h.value
        bad = b.copy()
        bad[0] ^= 1
        assert L.kfx_keyframes_import(kf._h, bad.ctypes.data, bad.size, C.byref(h)) == -1 and not h.value
        other.close()
    finally:
        st.close()
        kf.close()


# ---- 4. kfx_relocalise ----------------------------------------------------------

QUERIES = (4, 6, 7)


def model(dims, graph=1, overlap=True):
    """The scene's four frames fused, a keyframe added at each tracked pose."""
    intr, bgr, dep = frames8()
    kf = KinectFusion(Intrinsics.from_any(intr), VC.params(dims))
    kf.set_graph_mode(graph)
    kf.set_frame_overlap(overlap)
    st = Keyframes(kf)
    for k in range(4):
        assert kf.pipeline(bgr[k], dep[k]) == KFX_OK
        assert st.add() == k
    return kf, st


@functools.lru_cache(maxsize=None)
def oracle_poses(dims):
    intr, bgr, dep = frames8()
    pipe = O.Pipeline(Intrinsics.from_any(intr), VC.params(dims))
    for k in range(8):
        assert pipe.process(bgr[k], dep[k]) == 0
    return pipe.poses()


def composed(kf, st, k, starts, min_fitness):
    """kfx_relocalise from its parts: search, track_view per match, the restated selection."""
    matches = [m for m in st.search(None, k)[0].tolist() if m[0] >= 0]
    runs, cands = [], []
    for mi, (kid, dist) in enumerate(matches):
        res, world, q = kf.track_view(st.get(kid)[0], starts, quality=True)
        runs.append((res, world, q))
        cands += [R.candidate(q[s], mi, s) for s in range(len(starts)) if res[s].status == KFX_OK]
    want = RelocResult()
    want.status, want.keyframe, want.distance, want.start = KFX_TRACKING_LOST, -1, -1, -1
    want.n_matches, want.n_converged = len(matches), len(cands)
    best = R.select(cands)
    if best >= 0 and kfx.quality_figures(runs[cands[best][3]][2][cands[best][4]])[0] >= min_fitness:
        mi, s = cands[best][3], cands[best][4]
        want.status, want.keyframe, want.distance, want.start = KFX_OK, matches[mi][0], matches[mi][1], s
        want.world, want.icp, want.q = runs[mi][1][s], runs[mi][0][s], runs[mi][2][s]
    return want, cands


def _prev(kf):
    return [kf.frame_maps(KFX_FRAME_PREV, l)[1:] for l in range(kf.params.pyramid_height)]


def _same_maps(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for la, lb in zip(a, b) for x, y in zip(la, lb))


@pytest.mark.parametrize("dims", VC.DIMS)
def test_relocalise(dims):
    intr, bgr, dep = frames8()
    assert np.array_equal(bgr[:4], VC.scene()[1]) and np.array_equal(dep[:4], VC.scene()[2])
    kf, st = model(dims)
    try:
        kf.stage_icp()  # leaves its sums and step in DevState
        state = lambda: (kf.debug_get_icp_sums().tobytes(), kf.debug_get_icp_step().tobytes(),
                         kf.pose_record.tobytes(), kf.volume_checksum(), kf.frame_count)
        s0, m0 = state(), _prev(kf)
        ident = [Pose.identity()]
        for fr in QUERIES:
            kf.stage_preprocess(bgr[fr], dep[fr])
            for k, starts in ((4, ident), (2, M.starts(12))):
                got = kf.relocalise(st, k, None if starts is ident else starts, 0.0)
                want, cands = composed(kf, st, k, starts, 0.0)
                assert got.fields() == want.fields(), (fr, k)
                assert got.status == KFX_OK and got.n_matches == k and got.n_converged == len(cands) >= 1
                lost = kf.relocalise(st, k, None if starts is ident else starts, 1.1)
                assert lost.status == KFX_TRACKING_LOST and lost.keyframe == -1 and lost.start == -1
                assert (lost.n_matches, lost.n_converged) == (got.n_matches, got.n_converged)
                assert bytes(lost.world) == bytes(48) and lost.icp.solves == 0 and sum(lost.q.n) == 0
            # sanity, not parity: the accepted pose is nearer the tracked pose of that frame than the keyframe's
            got = kf.relocalise(st, 4, None, 0.0)
            tracked = oracle_poses(dims)[fr][:3, 3].astype(f32)
            a = np.linalg.norm(got.world.matrix()[:3, 3] - tracked)
            b = np.linalg.norm(st.get(got.keyframe)[0].matrix()[:3, 3] - tracked)
            print(dims, "frame", fr, "keyframe", got.keyframe, "distance", got.distance, "recovered", a, "keyframe", b,
                  "fitness", kfx.quality_figures(got.q)[0])
            if dims == 128:
                assert a < b
        assert state() == s0 and _same_maps(_prev(kf), m0)
        L = kfx.lib()
        out = RelocResult()
        C.memset(C.byref(out), 0xAB, C.sizeof(out))
        for k, n, fit in ((0, 1, 0.0), (17, 1, 0.0), (4, 1, float("nan"))):
            assert L.kfx_relocalise(kf._h, st._h, k, None, n, fit, C.byref(out)) == -1
        bad = (Pose * 1)(Pose.identity())
        bad[0].t[1] = float("inf")
        assert L.kfx_relocalise(kf._h, st._h, 4, bad, 1, 0.0, C.byref(out)) == -1
        assert L.kfx_relocalise(kf._h, st._h, 4, bad, 65537, 0.0, C.byref(out)) == -1
        assert L.kfx_relocalise(kf._h, st._h, 4, None, 1, 0.0, None) == -1
        assert bytes(out) == b"\xab" * C.sizeof(out)
    finally:
        st.close()
        kf.close()


def test_pending_tracking_status_is_left():
    intr, bgr, dep = frames8()
    kf, st = model(64)
    try:
        kf.pipeline_async(bgr[4], np.zeros_like(dep[4]))  # no depth: the frame is dropped
        code = st.encode()
        assert st.search([code], 2).shape == (1, 2, 2)
        assert kf.relocalise(st, 2, None, 0.0).status == KFX_TRACKING_LOST  # the reset left no model
        assert kf.synchronize() == KFX_TRACKING_LOST
        assert kf.synchronize() == KFX_OK
    finally:
        st.close()
        kf.close()


# ---- 5. kfx_pipeline_recover ----------------------------------------------------

@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("graph", [0, 1])
def test_recover_tracks_like_pipeline(graph, overlap):
    """Six tracked frames through kfx_pipeline and through kfx_pipeline_recover end alike; the keyframes added
    are the restated harvest."""
    intr, bgr, dep = frames8()
    par = RecoverParams(4, 3, 0.0, 0.2)
    made = []
    for _ in range(2):
        kf = KinectFusion(Intrinsics.from_any(intr), VC.params(64))
        kf.set_graph_mode(graph)
        kf.set_frame_overlap(overlap)
        made.append(kf)
    plain, rec = made
    st = Keyframes(rec)
    tab = st.table()
    try:
        held, events, added, want_added = [], [], [], []
        for k in range(6):
            assert plain.pipeline(bgr[k], dep[k]) == KFX_OK
            fit = kfx.quality_figures(plain.frame_quality(0))[0]
            code = R.encode(bgr[k], coarse(plain), tab, 4)
            take = (k == 0 or fit >= par.harvest_min_fitness) and (
                not held or R.search([code], held, 1)[0, 0, 1] > par.harvest_min_distance)
            want_added.append(len(held) if take else -1)
            if take:
                held.append(code)
            rc, rep = rec.pipeline_recover(st, bgr[k], dep[k], par)
            assert rc == KFX_OK and rep.reloc.keyframe == -1 and rep.reloc.status == KFX_OK
            events.append(rep.event)
            added.append(rep.keyframe_added)
        print("harvested", added)
        assert events == [1, 0, 0, 0, 0, 0] and added == want_added and added[0] == 0 and len(st) == len(held)
        assert len(held) >= 2  # (a condition on the inputs: the harvest adds more than the bootstrap frame)
        assert np.array_equal(plain.pose_record.view(np.uint32), rec.pose_record.view(np.uint32))
        assert _same_maps(_prev(plain), _prev(rec)) and plain.volume_checksum() == rec.volume_checksum()
        assert plain.frame_count == rec.frame_count == 7
    finally:
        st.close()
        plain.close()
        rec.close()


def test_recover_keeps_the_map_when_kidnapped():
    intr, bgr, dep = frames8()
    kf, st = model(64)
    twin, st2 = model(64)
    try:
        empty = KinectFusion(Intrinsics.from_any(intr), VC.params(64))
        nothing = empty.volume_checksum()
        empty.close()
        before = (kf.volume_checksum(), kf.pose_record.tobytes(), kf.frame_count, len(st))
        assert before[0] != nothing
        blank = np.zeros_like(dep[4])
        assert twin.pipeline(bgr[4], blank) == KFX_TRACKING_LOST and twin.volume_checksum() == nothing
        rc, rep = kf.pipeline_recover(st, bgr[4], blank, RecoverParams(4, 51, 0.0, 0.5))
        assert rc == KFX_TRACKING_LOST and rep.event == 3 and rep.keyframe_added == -1
        assert rep.reloc.status == KFX_TRACKING_LOST and rep.reloc.keyframe == -1 and rep.reloc.n_converged == 0
        assert (kf.volume_checksum(), kf.pose_record.tobytes(), kf.frame_count, len(st)) == before
        rc, rep = kf.pipeline_recover(st, bgr[4], dep[4], RecoverParams(4, 51, 0.0, 0.5))  # and goes on
        assert rc == KFX_OK and rep.event == 0
    finally:
        for x in (st, st2, kf, twin):
            x.close()


def miss_pose(kf):
    return dict((n, pose) for n, _, pose in VC.views(kf.pose_record[-1]))["miss"]


@pytest.mark.parametrize("graph", [0, 1])
def test_recover_relocalises_from_a_wrong_pose(graph):
    intr, bgr, dep = frames8()
    par = RecoverParams(4, 51, 0.0, 0.5)
    kf, st = model(64, graph)
    twin, st2 = model(64, graph)
    try:
        miss = miss_pose(kf)
        for x in (kf, twin):
            x.resume_at(miss)  # PREV is now empty: the next frame cannot track
        twin.stage_preprocess(bgr[4], dep[4])
        assert twin.stage_icp()[0] == KFX_TRACKING_LOST
        hand = twin.relocalise(st2, par.k, None, par.min_fitness)
        assert hand.status == KFX_OK
        twin.resume_at(hand.world)
        assert twin.pipeline(bgr[4], dep[4]) == KFX_OK
        rc, rep = kf.pipeline_recover(st, bgr[4], dep[4], par)
        assert rc == KFX_OK and rep.event == 2
        assert rep.reloc.fields() == hand.fields()
        assert np.array_equal(kf.pose_record.view(np.uint32), twin.pose_record.view(np.uint32))
        assert len(kf.pose_record) == 7 and kf.volume_checksum() == twin.volume_checksum()
        rc, rep = kf.pipeline_recover(st, bgr[5], dep[5], par)
        assert rc == KFX_OK and rep.event == 0 and rep.reloc.keyframe == -1
    finally:
        for x in (st, st2, kf, twin):
            x.close()


def test_runner_logs_recover(tmp_path):
    """kfx_run's fifteenth argument: one line per frame, the events of a short dataset with a blank depth frame."""
    import os
    import subprocess
    import pngw
    runner = os.path.join(os.path.dirname(kfx.LIB_PATH), "kfx_run")
    intr, bgr, dep = frames8()
    bgr, dep = bgr[:5], dep[:5].astype(np.uint16)
    dep[3] = 0
    root = str(tmp_path / "ds")
    os.makedirs(os.path.join(root, "color"))
    os.makedirs(os.path.join(root, "depth"))
    for k in range(len(dep)):
        pngw.write_png(os.path.join(root, "color", f"{k:06d}.png"), bgr[k][:, :, ::-1], 8, 2)
        pngw.write_png(os.path.join(root, "depth", f"{k:06d}.png"), dep[k], 16, 0)
    with open(os.path.join(root, "intr.txt"), "w") as f:
        f.write(f"{intr.fx} 0 {intr.cx}\n0 {intr.fy} {intr.cy}\n0 0 1\n")
    ds = kfx.Dataset(root)
    kf = KinectFusion(ds.intrinsics, default_params())  # the runner's parameters
    st = Keyframes(kf)
    want = []
    for k in range(len(ds)):
        c, d = ds.read(k)
        rc, rep = kf.pipeline_recover(st, c, d)
        fit = 0.0 if rep.event == 3 else kfx.quality_figures(kf.frame_quality(0))[0]
        want.append("%d %d %d %d %d %.9g" % (k, rep.event, rep.keyframe_added, rep.reloc.keyframe, rep.reloc.distance, fit))
    held = len(st)
    st.close()
    kf.close()
    ds.close()
    log = str(tmp_path / "recover.txt")
    r = subprocess.run([runner, root, str(tmp_path / "poses.txt")] + [""] * 12 + [log], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = open(log).read().splitlines()
    assert lines == want and [int(ln.split()[1]) for ln in lines] == [1, 0, 0, 3, 0]
    assert f"recover: {held} keyframes" in r.stdout and "end! 5 frames, frame_count 5" in r.stdout


def test_recover_refusals():
    """A candidate below min_fitness: event 3, the volume unchanged.  One slab of two: refused."""
    intr, bgr, dep = frames8()
    kf, st = model(64)
    try:
        kf.resume_at(miss_pose(kf))
        before = (kf.volume_checksum(), kf.pose_record.tobytes(), kf.frame_count)
        rc, rep = kf.pipeline_recover(st, bgr[4], dep[4], RecoverParams(4, 51, 1.1, 0.5))
        assert rc == KFX_TRACKING_LOST and rep.event == 3 and rep.reloc.keyframe == -1 and rep.reloc.n_converged >= 1
        assert (kf.volume_checksum(), kf.pose_record.tobytes(), kf.frame_count) == before
        L = kfx.lib()
        rep = kfx.abi.RecoverReport()
        assert L.kfx_pipeline_recover(kf._h, st._h, None, None, None, C.byref(rep)) == -1
        assert L.kfx_pipeline_recover(kf._h, st._h, kfx.abi.u8ptr(bgr[4]), kfx.abi.fptr(dep[4]), None, None) == -1
        bad = RecoverParams(0, 51, 0.0, 0.5)
        assert L.kfx_pipeline_recover(kf._h, st._h, kfx.abi.u8ptr(bgr[4]), kfx.abi.fptr(dep[4]), C.byref(bad),
                                      C.byref(rep)) == -1
        slab = KinectFusion(Intrinsics.from_any(intr), VC.params(64), slab=(0, 2))
        sst = Keyframes(slab)
        assert L.kfx_pipeline_recover(slab._h, sst._h, kfx.abi.u8ptr(bgr[0]), kfx.abi.fptr(dep[0]), None,
                                      C.byref(rep)) == -4
        out = RelocResult()
        assert L.kfx_relocalise(slab._h, sst._h, 4, None, 1, 0.0, C.byref(out)) == -4
        sst.close()
        slab.close()
    finally:
        st.close()
        kf.close()
