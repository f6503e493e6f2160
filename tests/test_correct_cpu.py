"""The frame correction without a GPU: that the numpy model (tests/correct_model.py) and the cases the GPU test runs
tell each listed mistake from the right answer; that the model's gray-world correction undoes the reference's failure
case 1 (a blue-deficient cast, README.md:325-342, :380-429) for the HSV extractor of tests/follow_model.py; and the
argument checks of unet_correct_u8_batch through the built library, which refuses before any device is touched."""
import ctypes as C

import numpy as np
import pytest

import correct_model as CM
import follow_model as FM
from unet_lane_detection_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---- 1. the model discriminates ------------------------------------------------------------------------------------

_right = {}


def _answer(name, bgr, mistakes=()):
    frames, cfg, extras = CM.case(name)
    padded = CM.padded_rows(frames, 3 * frames.shape[2] + extras["stride"]) if extras.get("stride") else None
    if not mistakes:
        if (name, bgr) not in _right:
            _right[(name, bgr)] = CM.correct(frames, cfg, bgr)
        return _right[(name, bgr)]
    return CM.correct(frames, cfg, bgr, mistakes=mistakes, padded=padded)


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("mistake", CM.MISTAKES)
def test_the_cases_tell_the_mistake_apart(mistake):
    told = [(name, bgr) for name in CM.CASES for bgr in (True, False)
            if not _same(_answer(name, bgr), _answer(name, bgr, (mistake,)))]
    print(mistake, "is told apart by", told)
    assert told, mistake
    # and it changes what the caller gets, not only an intermediate
    assert any(not np.array_equal(_answer(n, b)["out"], _answer(n, b, (mistake,))["out"]) for n, b in told), mistake


def test_the_model_on_hand_made_frames():
    """a flat frame: the stretch finds hi <= lo and is not applied, the one full bin is clipped to L and spread"""
    frames, cfg, _ = CM.case("flat_300x300")
    res = CM.correct(frames, cfg)
    assert res["hist"][0, :, 93].tolist() == [90000] * 3 and res["plan"][0, 1:4].tolist() == [65536] * 3
    assert res["plan"][0, 0] == CM.FLAG_CORRECTED | CM.FLAG_CLAHE and res["plan"][0, 4] == res["plan"][0, 5] == 93
    level = int(CM.TONE[93])
    assert int(res["tile_hist"][0, 0, 0, level]) == 90000         # 16 bits would hold 24464
    # L = 512 * 90000 / 65536 = 703, E = 89297: every bin gets 348, the first 209 one more
    table = res["tile_lut"][0, 0, 0].astype(np.int64)
    cdf = lambda i: 348 * (i + 1) + min(i + 1, 209) + (703 if i >= level else 0)
    assert table.tolist() == [(255 * cdf(i) + 45000) // 90000 for i in range(256)] and table[255] == 255
    assert (res["out"] == table[level]).all()
    # the gate: a normal frame passes through, and nothing but S is recorded
    f, cfg, _ = CM.case("only_flagged")
    res = CM.correct(f, cfg)
    assert res["plan"][:, 0].tolist() == [7, 0, 7] and np.array_equal(res["out"][1], f[1])
    assert not np.array_equal(res["out"][0], f[0]) and not res["tile_hist"][1].any()
    s = int(f[1].astype(np.int64).sum())
    assert res["plan"][1].tolist() == [0, 65536, 65536, 65536, 0, 255, s & 0xFFFFFFFF, s >> 32]
    # the gain clamps of the gain case: unity for an empty channel, max_gain and 1 / max_gain
    f, cfg, _ = CM.case("gain_clamp")
    plan = CM.correct(f, cfg)["plan"]
    assert plan[0, 2] == 65536 and plan[1, 1] == 2 * 65536 and plan[2, 3] == 65536 // 2


def test_grids_that_leave_a_tile_empty():
    assert not CM.grid_fits(9, 64, 1, 8) and CM.grid_fits(9, 64, 1, 5) and CM.grid_fits(16, 16, 16, 16)
    assert all(CM.grid_fits(f.shape[1], f.shape[2], kw.get("grid_x", 1), kw.get("grid_y", 1))
               for f, kw, _ in CM.CASES.values())


# ---- 2. the reference's failure case 1 -----------------------------------------------------------------------------

def test_gray_world_undoes_a_blue_deficient_cast():
    clean = CM.track()
    bad = CM.cast(clean)
    want = FM.hsv_lanes(clean[None])[0]
    assert want.any() and not want.all()
    assert not FM.hsv_lanes(bad[None]).any()                      # the extractor finds no lane pixel at all
    res = CM.correct(bad[None], CM.config(white_balance=1))
    assert np.array_equal(FM.hsv_lanes(res["out"])[0], want)       # bit for bit the mask of the uncast frame
    # every level is at least 16 away from the extractor's thresholds (S <= 40, V >= 185), in all three states
    from unet_lane_detection_amd.augment import rgb_to_hsv
    for img, lane_state in ((clean, True), (bad, False), (res["out"][0], True)):
        hsv = rgb_to_hsv(img[..., ::-1]).astype(np.int64)
        lane = (clean[..., 0] == CM.TRACK_WHITE)
        assert (hsv[~lane][:, 2] <= 185 - 16).all()
        assert (hsv[lane][:, 2] >= 185 + 16).all()
        assert ((hsv[lane][:, 1] <= 40 - 16) if lane_state else (hsv[lane][:, 1] >= 40 + 16)).all()
    gains = res["plan"][0, 1:4].astype(np.float64) / 65536
    print("gains (B, G, R):", gains)
    assert gains[0] > 1.2 and gains[1] < 1.0 and gains[1] == gains[2]


# ---- 3. the ABI, without a device ----------------------------------------------------------------------------------

def _cfg(**kw):
    m = CM.config(**kw)
    s = _lib.CorrectConfigStruct()
    for k, v in m.items():
        if k == "tone":
            C.memmove(s.tone, v.ctypes.data, 256)
        else:
            setattr(s, k, v)
    return s


def test_struct_and_work_sizes(lib):
    assert lib.unet_correct_config_bytes() == C.sizeof(_lib.CorrectConfigStruct) == 11 * 4 + 256
    for n, gx, gy in ((1, 1, 1), (3, 4, 3), (64, 8, 8), (2, 16, 16)):
        layout = n * (3 * 256 * 4 + 8 * 4 + 3 * 256 + gy * gx * 256 * 4 + gy * gx * 256)
        assert lib.unet_correct_work_bytes(n, gx, gy) == layout == CM.work_bytes(n, gx, gy)
    assert lib.unet_correct_work_bytes(0, 1, 1) == 0 and lib.unet_correct_work_bytes(1, 17, 1) == 0


def test_bad_arguments_are_refused_before_a_device_is_touched(lib):
    name = b"unet_correct_u8_batch"
    buf = (C.c_uint8 * 4096)()
    frames, out, work = C.c_void_p(C.addressof(buf)), C.c_void_p(C.addressof(buf) + 2048), C.c_void_p(C.addressof(buf) + 1024)
    big = 1 << 40

    def call(frames=frames, n=1, h=16, w=16, stride=0, bgr=1, cfg=None, out=out, ostride=0, work=work, wbytes=big,
             device=0):
        cfg = C.byref(cfg if cfg is not None else _cfg(grid_x=2, grid_y=2)) if cfg is not False else None
        return lib.unet_correct_u8_batch(device, frames, n, h, w, stride, bgr, cfg, out, ostride, work, wbytes, None)

    def refused(rc, word=None):
        msg = lib.unet_op_last_error()
        return rc == 1 and msg.startswith(b"invalid argument") and name in msg and (word is None or word in msg)

    assert refused(call(frames=None), b"null") and refused(call(out=None), b"null")
    assert refused(call(work=None), b"null") and refused(call(cfg=False), b"null")
    assert refused(call(stride=47), b"row_stride") and refused(call(ostride=47), b"out_row_stride")
    assert refused(call(n=0)) and refused(call(h=0)) and refused(call(w=16385)) and refused(call(h=16385))
    for g in (0, 17):
        assert refused(call(cfg=_cfg(grid_x=g)), b"grid") and refused(call(cfg=_cfg(grid_y=g, clahe=1)), b"grid")
    assert refused(call(h=9, cfg=_cfg(grid_y=8)), b"empty")           # ceil(9 / 8) = 2 rows a tile: 7 * 2 >= 9
    assert refused(call(w=9, cfg=_cfg(grid_x=8, clahe=1)), b"empty")
    assert refused(call(cfg=_cfg(max_gain=0)), b"max_gain") and refused(call(cfg=_cfg(max_gain=9)), b"max_gain")
    assert refused(call(n=1 << 17, h=128, w=128), b"2^31")            # exactly 2^31 pixels
    assert refused(call(n=8, h=1 << 14, w=1 << 14), b"2^31") and refused(call(n=1 << 11, h=1 << 10, w=1 << 10), b"2^31")
    assert refused(call(cfg=_cfg(white_balance=2)), b"white_balance")
    assert refused(call(cfg=_cfg(lo_bp=-1))) and refused(call(cfg=_cfg(lo_bp=5000, hi_bp=5000)), b"lo_bp")
    assert refused(call(cfg=_cfg(clip_q8=0)), b"clip_q8")
    assert refused(call(cfg=_cfg(dark_limit=201)), b"dark_limit")
    assert refused(call(wbytes=CM.work_bytes(1, 2, 2) - 1), b"work_bytes")
    assert refused(call(work=C.c_void_p(C.addressof(buf) + 1025)), b"aligned")
    assert refused(call(out=frames, stride=48, ostride=64), b"in place")
    assert refused(call(out=C.c_void_p(C.addressof(buf) + 100)), b"overlaps")
    assert not any(buf)
    # what passes the checks goes on to the device: an ordinal the runtime refuses shows it got that far
    for kw in (dict(), dict(out=frames), dict(stride=50, ostride=64), dict(h=9, cfg=_cfg(grid_y=5, clahe=1)),
               dict(n=(1 << 17) - 1, h=128, w=128, out=frames)):
        assert call(device=1 << 20, **kw) == _lib.UNET_ERR_HIP
        assert b"hipSetDevice" in lib.unet_op_last_error()
    assert not any(buf)


def test_config_objects():
    from unet_lane_detection_amd import correct as K
    s = K.CorrectConfig().struct()
    assert (s.white_balance, s.max_gain, s.lo_bp, s.hi_bp, s.clahe, s.grid_x, s.grid_y, s.clip_q8, s.only_flagged,
            s.dark_limit, s.bright_limit) == (1, 4, 0, 0, 0, 1, 1, 512, 0, 50, 200)
    assert bytes(s.tone) == bytes(range(256))
    s = K.CorrectConfig(white_balance=None, stretch=(1.0, 0.5), gamma=0.8, clahe=K.Clahe(3.0, (4, 3)), max_gain=2,
                        only_flagged=True).struct()
    assert (s.white_balance, s.max_gain, s.lo_bp, s.hi_bp, s.clahe, s.grid_x, s.grid_y, s.clip_q8,
            s.only_flagged) == (0, 2, 100, 50, 1, 4, 3, 768, 1)
    assert np.array_equal(np.frombuffer(bytes(s.tone), np.uint8), CM.gamma_table(0.8))
    assert np.array_equal(K.gamma_table(0.8), CM.TONE) and K.Clahe().grid == (8, 8) and K.Clahe().clip_limit == 2.0
    with pytest.raises(ValueError):
        K.CorrectConfig(white_balance="retinex").struct()
    with pytest.raises(ValueError):
        K.CorrectConfig(gamma=0.5, tone=np.arange(256, dtype=np.uint8)).struct()
