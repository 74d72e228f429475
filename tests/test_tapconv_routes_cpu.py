"""The dispatcher of bcos_tapconv_ops against the case table (tests/tapconv_cases.py), without a device: the route query
(include/bcos_hip.h: bcos_tapconv_route_query) runs the launch path's own planning functions and launches nothing.

  * every case takes the launcher, loop and epilogue kind the table expects, under the options the case sets;
  * the table is complete: every (route, loop, direction, epilogue kind) the library can report is reached by a case or listed as
    unreachable with the source line that makes it so -- a launcher nobody tests is a failure, and so is a stale exemption;
  * the query is pure, and rejects what the launch rejects with the launch's error code;
  * the image-range question (bcos_tapconv_fuses_image_range) is answered by the rule the header documents, for every case.
"""
import ctypes as C

import pytest
import torch

import tapconv_cases as tc


@pytest.fixture(scope="module")
def blib(hip_lib):
    from bcos_hip import lib
    return lib


def _query(blib, case):
    b = tc.Built(case, "cpu", blib)
    with tc.with_options(blib, b.options()):
        return blib.route_query(b.ops, b.geom, b.epi), b


def test_case_ids_are_unique():
    ids = [c.id for c in tc.CASES]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.id)
def test_case_takes_the_expected_route(blib, case):
    q, _ = _query(blib, case)
    r = case.r
    assert (q["route"], q["loop"], q["epi_kind"], q["norm"]) == (r.route, r.loop, case.kind, int(case.e.norm)), (case.id, q)
    assert q["chunks"] == r.chunks and q["ch_pass"] == r.ch_pass, (case.id, q)
    if r.route != "skinny":
        bm, bn = (int(v) for v in r.route.split("_")[1].split("x"))
        assert (q["bm"], q["bn"]) == (bm, bn)


def _reached(blib):
    out = {}
    for case in tc.CASES:
        q, _ = _query(blib, case)
        out.setdefault((q["route"], q["loop"], q["norm"], q["epi_kind"]), []).append(case.id)
    return out


def test_every_route_loop_and_epilogue_kind_is_reached_or_listed(blib):
    lib = blib.load()
    assert lib.bcos_tapconv_epilogue_kinds() == tc.N_KINDS
    names = blib.route_names()
    assert len(names) == lib.bcos_tapconv_route_count() and len(set(names)) == len(names) and "skinny" in names
    assert lib.bcos_tapconv_route_name(len(names)) is None and lib.bcos_tapconv_route_name(-1) is None
    reached = _reached(blib)
    listed = {(route, norm, kind) for route, norm, kind, _why in tc.UNREACHABLE}
    assert all(why for *_x, why in tc.UNREACHABLE)
    missing, stale = [], []
    for route in names:
        for loop in tc.loops_of(route):
            for norm in (0, 1):
                for kind in range(tc.N_KINDS + 1):
                    hit = (route, loop, norm, kind) in reached
                    if (route, norm, kind) in listed:
                        if hit:
                            stale.append((route, loop, norm, kind))
                    elif not hit:
                        missing.append((route, loop, norm, kind))
    assert not missing, f"(route, loop, B-cos launch, epilogue kind) neither reached by a case nor listed in UNREACHABLE: {missing}"
    assert not stale, f"listed in UNREACHABLE, yet reached: {stale}"
    unknown = {k[0] for k in reached} - set(names)
    assert not unknown, unknown


def test_shapes_of_the_table_are_ragged():
    """conditions the table sets for itself: rows not a multiple of 32, at least two row tiles, a row tile shared by two images;
    column counts off the tile width; a K that is not a multiple of 64 and C % 16 != 0 where the launcher's guard allows"""
    by_route = {}
    for r in tc.ROUTES:
        by_route.setdefault(r.route, []).append(r)
        if r.route == "skinny":
            continue
        bm, bn = (int(v) for v in r.route.split("_")[1].split("x"))
        assert r.M % 32 != 0, r.name
        assert r.M > bm, r.name
        two_d = r.route.startswith("p2_")                        # 2-D row tiles never span images
        assert two_d or (r.P * r.Q) % bm != 0, r.name            # some tile holds rows of two images
        assert max(r.groups, 1) * r.Cout % bn != 0 or r.name in ("d192_576", "cfg128_groups_presplit"), r.name
        assert (r.k * r.k * r.C) % 64 != 0 or r.k == 4 or r.aligned, r.name       # (16 taps of C % 4 == 0 channels: always a multiple of 64)
    for route, rs in by_route.items():
        if route.split("_")[0] in ("cfg", "h2", "d") and not route.endswith("256x32"):
            assert any(r.C % 16 != 0 for r in rs), route        # the uniform_tap = 0 walk (patch launchers need C % 16 == 0)
    # ... and the aligned walks are launched too: C % 32 == 0 (uniform_tap = 1) on every non-patch family, the channel-chunk-major K walk of the
    # LDS-DMA loop (2 .. 16 taps, C % 16 == 0, no image maxima), and Cout % 4 != 0 on every family and on the narrow kernel
    fam = lambda r: r.route.split("_")[0]
    for f in ("cfg", "h2", "d"):
        assert any(fam(r) == f and r.C % 32 == 0 and r.k == 1 for r in tc.ROUTES), f
        assert any(fam(r) == f and r.C % 16 == 0 and 1 < r.k * r.k <= 16 and not r.imgmax for r in tc.ROUTES), f
    for f in ("cfg", "h2", "d", "p", "p2", "skinny"):
        assert any(fam(r) == f and r.Cout % 4 != 0 for r in tc.ROUTES), f
    assert {r.ch_pass == r.C for r in by_route["skinny"]} == {True, False}      # one pass over all channels, and channel slices


@pytest.mark.parametrize("detour", tc.FEATURE_DETOURS, ids=lambda d: f"{d[0]}-{d[1].name}")
def test_features_the_dispatcher_keeps_off_a_launcher(blib, detour):
    name, epi, instead, why = detour
    r = next(x for x in tc.ROUTES if x.name == name)
    q, _ = _query(blib, tc.Case(r, epi))
    assert q["route"] != r.route and q["route"] == instead, (q, why)


def test_image_range_answer_follows_the_documented_rule(blib):
    """include/bcos_hip.h: the launch folds the per-image range of its out_absmax itself iff it takes a specialised epilogue, emits
    out_absmax, maps its output plainly (no depth to space), has one group and at least 19 rows per image"""
    lib = blib.load()
    wrong = []
    for case in tc.CASES:
        r = case.r
        b = tc.Built(case, "cpu", blib)
        args = (C.byref(b.ops), C.byref(b.geom), C.byref(b.epi))
        expect = int(case.kind > 0 and case.absmax and not r.cgroup and max(r.groups, 1) == 1 and r.P * r.Q >= 19)
        with tc.with_options(blib, b.options()):
            got = lib.bcos_tapconv_fuses_image_range(*args)
        if got != expect:
            wrong.append((case.id, got, expect))
        if r.name in ("cfg64_chunks", "d64_chunks"):        # the batch-chunk path answers what the unchunked call answers
            assert "split_limit" in b.options()
            with tc.with_options(blib, {k: v for k, v in b.options().items() if k != "split_limit"}):
                assert lib.bcos_tapconv_fuses_image_range(*args) == got, case.id
    assert not wrong, wrong
    assert {r.name for r in tc.ROUTES if dict(r.opts).get("split_limit")} == {"cfg64_chunks", "d64_chunks"}


def test_query_is_pure_and_leaves_the_options_alone(blib):
    lib = blib.load()
    case = next(c for c in tc.CASES if c.id == "d256-f1_relu_scale")
    b = tc.Built(case, "cpu", blib)
    before = {n: blib.get_option(n) for n in blib.OPTIONS}
    mode = lib.bcos_get_contraction_mode()
    structs = [bytes(memoryview(s)) for s in (b.ops, b.geom, b.epi)]
    with tc.with_options(blib, b.options()):
        inside = {n: blib.get_option(n) for n in blib.OPTIONS}
        answers = [blib.route_query(b.ops, b.geom, b.epi) for _ in range(3)]
        assert {n: blib.get_option(n) for n in blib.OPTIONS} == inside
    assert answers[0] == answers[1] == answers[2] and answers[0]["route"] == "d_128x256"
    assert {n: blib.get_option(n) for n in blib.OPTIONS} == before and lib.bcos_get_contraction_mode() == mode
    assert [bytes(memoryview(s)) for s in (b.ops, b.geom, b.epi)] == structs       # the arguments are not written to
    # the answer follows the option table of the moment: without the forced tile width this few-row launch takes the narrow column tiles
    assert blib.route_query(b.ops, b.geom, b.epi)["route"] == "d_128x32"
    # ... and a query does not leave the image-range query or a later launch validation in query mode
    assert lib.bcos_tapconv_fuses_image_range(C.byref(b.ops), C.byref(b.geom), C.byref(b.epi)) in (0, 1)


def test_query_rejects_what_the_launch_rejects(blib):
    """the argument cases of tests/asan/abi_validation.c: the query returns bcos_tapconv_ops' own error code (nothing reaches a device:
    every one of them is rejected ahead of the launch)"""
    lib = blib.load()
    E_INVAL, E_NOSUP = -22, blib.BCOS_E_NOSUP
    buf = torch.zeros(1024)
    p = buf.data_ptr()
    assert p % 16 == 0

    def fresh():
        g = blib.TapconvGeom()
        for k, v in dict(N=1, H=4, W=4, C=8, P=4, Q=4, in_sh=1, in_sw=1, dstep_h=1, dstep_w=1, TH=1, TW=1, OH=4, OW=4, out_sh=1, out_sw=1, Cout=8).items():
            setattr(g, k, v)
        e = blib.Epilogue()
        e.out, e.b = p, 2.0
        o = blib.Operands()
        o.a, o.wt = p, p
        return o, g, e

    def both(o, g, e, code):
        r = blib.TapconvRoute()
        rc_q = lib.bcos_tapconv_route_query(C.byref(o), C.byref(g), C.byref(e), C.byref(r))
        rc_l = lib.bcos_tapconv_ops(C.byref(o), C.byref(g), C.byref(e), None)
        assert rc_q == rc_l == code, (rc_q, rc_l, code)
        assert lib.bcos_last_error_string()

    o, g, e = fresh()
    r = blib.TapconvRoute()
    assert lib.bcos_tapconv_route_query(None, C.byref(g), C.byref(e), C.byref(r)) == E_INVAL
    assert lib.bcos_tapconv_route_query(C.byref(o), None, C.byref(e), C.byref(r)) == E_INVAL
    assert lib.bcos_tapconv_route_query(C.byref(o), C.byref(g), None, C.byref(r)) == E_INVAL
    assert lib.bcos_tapconv_route_query(C.byref(o), C.byref(g), C.byref(e), None) == E_INVAL
    edits = [
        (lambda o, g, e: setattr(o, "a", None), E_INVAL),
        (lambda o, g, e: setattr(o, "contraction", 7), E_INVAL),
        (lambda o, g, e: setattr(g, "C", 6), E_INVAL),
        (lambda o, g, e: setattr(g, "Cout", 0), E_INVAL),
        (lambda o, g, e: setattr(o, "a", p + 4), E_INVAL),
        (lambda o, g, e: setattr(e, "out", None), E_INVAL),
        (lambda o, g, e: setattr(g, "out_h0", 9), E_INVAL),
        (lambda o, g, e: setattr(g, "a_pitch", 6), E_INVAL),
        (lambda o, g, e: setattr(g, "out_pitch", 4), E_INVAL),
        (lambda o, g, e: setattr(e, "addend_sub", 2), E_INVAL),
        (lambda o, g, e: setattr(e, "addend_sub", -1), E_INVAL),
        (lambda o, g, e: setattr(e, "a_sumsq", p), E_INVAL),
        (lambda o, g, e: setattr(g, "out_cgroup", 4), E_INVAL),
        (lambda o, g, e: setattr(e, "rowadd", p), E_NOSUP),
        (lambda o, g, e: (setattr(e, "out_imgmax", p), setattr(e, "out_imgmin_c", p + 64)), E_NOSUP),
        (lambda o, g, e: setattr(e, "max_out", 3), E_NOSUP),
    ]
    for edit, code in edits:
        o, g, e = fresh()
        edit(o, g, e)
        both(o, g, e, code)
    # a valid call is answered and the answer is filled in
    o, g, e = fresh()
    assert lib.bcos_tapconv_route_query(C.byref(o), C.byref(g), C.byref(e), C.byref(r)) == 0
    assert lib.bcos_tapconv_route_name(r.route) == b"skinny" and r.ch_pass == 8 and r.chunks == 1
