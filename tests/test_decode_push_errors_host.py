"""The error contract of the decode stream and the listener group as a whole (emagls_decode_stream_* / emagls_decode_group_*): a
fixed table of bad and borderline argument lists, each with the status and the full text of emagls_last_error() that the library
gave when the table was recorded (tests/golden/decode_push_errors.json).  The statuses and the texts are part of the ABI, and so is
which error a call with two of them reports.  Through ctypes, and no call of the table reaches a device.

The table is recorded by hand, never by the test:  EMAGLS_RECORD_DECODE_PUSH_ERRORS=1 python tests/test_decode_push_errors_host.py"""
import ctypes as C
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_push_errors.json")
SH, CH, REAL = 0, 1, 0

# the objects the calls of the table are made on: kind, channels, sets, taps, block, layout, listeners, microphones (0: not encoded)
OBJECTS = {
    "stream": dict(kind="stream", nch=4, n_sets=2, len=100, block=64, layout=SH, listeners=1, nmics=0),
    "group": dict(kind="group", nch=4, n_sets=2, len=100, block=64, layout=SH, listeners=3, nmics=0),
    "group_of_one": dict(kind="group", nch=4, n_sets=2, len=100, block=64, layout=SH, listeners=1, nmics=0),
    "stream_ch": dict(kind="stream", nch=5, n_sets=1, len=8, block=64, layout=CH, listeners=1, nmics=0),
    "group_ch": dict(kind="group", nch=5, n_sets=1, len=8, block=64, layout=CH, listeners=2, nmics=0),
    "stream_no_square": dict(kind="stream", nch=5, n_sets=1, len=8, block=64, layout=SH, listeners=1, nmics=0),
    "group_no_square": dict(kind="group", nch=5, n_sets=1, len=8, block=64, layout=SH, listeners=2, nmics=0),
    "stream_order_16": dict(kind="stream", nch=289, n_sets=1, len=8, block=64, layout=SH, listeners=1, nmics=0),
    "group_order_16": dict(kind="group", nch=289, n_sets=1, len=8, block=64, layout=SH, listeners=2, nmics=0),
    "stream_encoded": dict(kind="stream", nch=4, n_sets=2, len=100, block=64, layout=SH, listeners=1, nmics=6),
    "group_encoded": dict(kind="group", nch=4, n_sets=2, len=100, block=64, layout=SH, listeners=3, nmics=6),
}


def _table():
    """(entry, object or None, arguments) of every call.  An array argument is [count, fill]: fill None is a null pointer."""
    t = []

    def create(entry, **kw):
        a = dict(nch=4, n_sets=1, len=8, block=64, layout=SH, basis=REAL, in_c=0, null_wL=False, null_wR=False, null_out=False)
        if "group" in entry:
            a["listeners"] = 3
        if "encoded" in entry:
            a.update(nmics=6, null_enc=False)
            del a["in_c"]
        a.update(kw)
        t.append((entry, None, a))

    def push(obj, nsamp, set=None, yaw=None, pitch=None, roll=None, **kw):
        group = obj is None and kw.pop("null_group", False) or (obj is not None and OBJECTS[obj]["kind"] == "group")
        a = dict(nsamp=nsamp, set=set or [0, None], yaw=yaw or [0, None], pitch=pitch or [0, None], roll=roll or [0, None], null_in=False,
                 null_out=False)
        a.update(kw)
        t.append(("group_push" if group else "push_sets", obj, a))

    for e in ("create_bank", "create_encoded", "group_create", "group_create_encoded"):
        create(e)                                   # a good one, for what a success leaves
        create(e, null_wL=True)
        create(e, null_wR=True)
        create(e, null_out=True)
        create(e, block=96)
        create(e, nch=1, len=16385)
        create(e, nch=1, len=16384, block=2048)
        create(e, n_sets=0)
        create(e, n_sets=65537)
        create(e, nch=0)
        create(e, len=0)
        create(e, layout=2)
        create(e, basis=2)
        create(e, n_sets=0, block=96)               # two at once: the sets are looked at first
        create(e, block=96, len=16385, nch=1)       # two at once
        create(e, layout=7, basis=7)                # two at once
    for e in ("group_create", "group_create_encoded"):
        for n in (0, -2, 4097, 4096):
            create(e, listeners=n)
        create(e, listeners=0, n_sets=0)            # two at once
        create(e, listeners=4097, block=96)         # two at once
    for e in ("create_encoded", "group_create_encoded"):
        for m in (0, 65, 64):
            create(e, nmics=m)
        create(e, null_enc=True)
        create(e, nch=65)
        create(e, nmics=0, null_enc=True)           # two at once
        create(e, null_enc=True, block=96)          # two at once
        create(e, nmics=65, null_wL=True)           # two at once
    create("group_create_encoded", nmics=0, listeners=0)

    # a null handle
    push(None, 64)
    push(None, 64, null_group=True)
    push(None, 100, set=[5, None], null_group=True)
    push(None, 100, set=[5, None])
    for s, g in (("stream", "group"), ("stream_encoded", "group_encoded")):
        L = OBJECTS[g]["listeners"]
        # the samples of a push
        for o in (s, g):
            push(o, 100)
            push(o, 0)
            push(o, -64)
            push(o, 0, yaw=[1, 0.5])
            push(o, 128, null_in=True)
            push(o, 128, null_out=True)
            push(o, 0, null_in=True)
        # each angle count off by one, and a null array with a positive count
        for ang in ("yaw", "pitch", "roll"):
            for n in (2, 127, 129, -1):
                push(s, 128, **{ang: [n, 0.25]})
            push(s, 128, **{ang: [1, None]})
            push(s, 128, **{ang: [128, None]})
            for n in (L - 1, L + 1, L * 128 - 1, L * 128 + 1, 128, 1, -1):   # 128, 1: one listener's worth
                push(g, 128, **{ang: [n, 0.25]})
            push(g, 128, **{ang: [L, None]})
            push(g, 128, **{ang: [L * 128, None]})
        # set counts off by one, a null array, indices outside the bank
        for n in (2, 3, 5, -1):
            push(s, 256, set=[n, 0])
        push(s, 256, set=[1, None])
        push(s, 256, set=[4, None])
        for n in (L - 1, L + 1, L * 4 - 1, L * 4 + 1, 4, 1, -1):
            push(g, 256, set=[n, 0])
        push(g, 256, set=[L, None])
        push(g, 256, set=[L * 4, None])
        for bad in (2, -1):
            push(s, 256, set=[1, bad])
            push(s, 256, set=[4, [0, 1, bad, 0]])
            push(s, 0, set=[1, bad])
            push(g, 256, set=[L, [0, bad, 1]])
            push(g, 256, set=[L * 4, [0, 1] * (2 * L - 1) + [0, bad]])
            push(g, 0, set=[L, [0, bad, 1]])
        # all-zero pitch with a roll count that does not fit, and the other way round
        push(s, 128, pitch=[128, 0.0], roll=[5, 0.0])
        push(s, 128, pitch=[5, 0.0], roll=[128, 0.0])
        push(s, 128, pitch=[128, 0.0], roll=[128, 0.0], yaw=[5, 0.0])
        push(g, 128, pitch=[L * 128, 0.0], roll=[L + 1, 0.0])
        push(g, 128, pitch=[L + 1, 0.0], roll=[L * 128, 0.0])
        push(g, 128, pitch=[L, 0.0], roll=[L, 0.0], yaw=[L + 1, 0.0])
        # two errors at once
        push(s, 100, set=[3, 0], yaw=[5, 0.25])               # samples, then the rest
        push(g, 100, set=[L + 1, 0], yaw=[L + 1, 0.25])
        push(s, 256, set=[3, 0], yaw=[5, 0.25])               # a set count and an angle count
        push(g, 256, set=[L + 1, 0], yaw=[L + 1, 0.25])
        push(s, 256, set=[3, 0], pitch=[5, 0.25])
        push(g, 256, set=[L + 1, 0], pitch=[L + 1, 0.25])
        push(s, 256, set=[4, None], yaw=[5, 0.25])            # a null set array and an angle count
        push(g, 256, set=[L, None], yaw=[L + 1, 0.25])
        push(s, 256, set=[1, 2], yaw=[5, 0.25])               # an index outside the bank and an angle count
        push(g, 256, set=[L, 2], yaw=[L + 1, 0.25])
        push(s, 256, set=[1, 2], null_in=True)                # an index outside the bank and a null block
        push(g, 256, set=[L, 2], null_in=True)
        push(s, 256, set=[3, 0], null_out=True)
        push(g, 256, set=[L + 1, 0], null_out=True)
        push(s, 256, yaw=[5, 0.25], pitch=[7, 0.25])          # two angle counts
        push(g, 256, yaw=[L + 1, 0.25], pitch=[L + 2, 0.25])
        push(g, 256, yaw=[L, None], pitch=[L + 2, 0.25])
        push(s, 256, yaw=[256, None], pitch=[7, 0.25])
        push(s, 256, yaw=[5, 0.25], null_in=True)
        push(g, 256, yaw=[L + 1, 0.25], null_in=True)
    # a group of one listener takes a stream's counts
    for n in (2, 127, 129):
        push("group_of_one", 128, yaw=[n, 0.25])
    for n in (2, 3, 5):
        push("group_of_one", 256, set=[n, 0])
    push("group_of_one", 256, set=[1, 2])
    # pitch on a CH layout; pitch with a channel count that is no square; an SH order above 15
    for s, g in (("stream_ch", "group_ch"), ("stream_no_square", "group_no_square"), ("stream_order_16", "group_order_16")):
        push(s, 64, pitch=[1, 0.1])
        push(s, 64, roll=[64, 0.1])
        push(s, 0, yaw=[1, 0.1])
        push(s, 0, pitch=[1, 0.0])                            # zeros are dropped: no rotation at all
        push(s, 0, pitch=[1, 0.0], yaw=[1, 0.1])              # ... or the yaw rotation, in its wording
        push(s, 64, pitch=[1, 0.0], yaw=[5, 0.1])
        push(s, 64, pitch=[1, 0.1], yaw=[5, 0.1])             # two at once
        push(s, 64, pitch=[1, 0.1], set=[1, 1])
        push(g, 64, pitch=[2, 0.1])
        push(g, 64, roll=[128, 0.1])
        push(g, 0, yaw=[2, 0.1])
        push(g, 0, pitch=[2, 0.0])
        push(g, 0, pitch=[2, 0.0], yaw=[2, 0.1])
        push(g, 64, pitch=[2, 0.1], yaw=[3, 0.1])
        push(g, 64, pitch=[2, 0.1], set=[2, 1])

    t.append(("group_reset", None, dict(listener=0)))
    t.append(("group_reset", None, dict(listener=-7)))
    for o in ("group", "group_of_one", "group_encoded"):
        for bad in (-2, OBJECTS[o]["listeners"], 4096):
            t.append(("group_reset", o, dict(listener=bad)))
    for null_outs in (False, True):
        t.append(("stream_info", None, dict(null_outs=null_outs)))
        t.append(("group_info", None, dict(null_outs=null_outs)))
        for o, d in OBJECTS.items():
            t.append(("group_info" if d["kind"] == "group" else "stream_info", o, dict(null_outs=null_outs)))
    for null_out in (False, True):
        t.append(("stream_sets", None, dict(null_out=null_out)))
        t.append(("stream_sets", "stream", dict(null_out=null_out)))
        t.append(("stream_sets", "stream_ch", dict(null_out=null_out)))
    t.append(("stream_destroy", None, {}))
    t.append(("group_destroy", None, {}))
    return t


def _zeros(count):
    return np.zeros(max(min(int(count), 1 << 24), 1))


def _create(lib, entry, a):
    """-> status, the handle (c_void_p), what the call left in *out ('null', 'set' or None when out is null)"""
    w = _zeros(a["n_sets"] * a["len"] * a["nch"])
    pw = w.ctypes.data_as(C.c_void_p)
    h = C.c_void_p(0xdead)      # a failed creation leaves null behind, whenever it was given somewhere to leave it
    out = None if a["null_out"] else C.byref(h)
    wl, wr = None if a["null_wL"] else pw, None if a["null_wR"] else pw
    tail = [a["listeners"]] if "group" in entry else []
    if "encoded" in entry:
        enc = _zeros(a["nch"] * a["nmics"])
        pe = None if a["null_enc"] else enc.ctypes.data_as(C.c_void_p)
        f = lib.emagls_decode_group_create_encoded if "group" in entry else lib.emagls_decode_stream_create_encoded
        rc = f(a["nmics"], pe, 0, a["nch"], a["n_sets"], wl, wr, 0, a["len"], a["layout"], a["basis"], a["block"], *tail, out)
    else:
        f = lib.emagls_decode_group_create if "group" in entry else lib.emagls_decode_stream_create_bank
        rc = f(a["nch"], a["n_sets"], wl, wr, 0, a["len"], a["in_c"], a["layout"], a["basis"], a["block"], *tail, out)
    if a["null_out"] or h.value == 0xdead:
        return rc, C.c_void_p(), None if a["null_out"] else "untouched"
    return rc, h, "set" if h.value else "null"


def _array(spec, dtype):
    count, fill = spec
    if fill is None:
        return None, None, count
    v = np.ascontiguousarray(np.broadcast_to(np.asarray(fill, dtype=dtype).reshape(-1), (max(count, 1),)) if np.ndim(fill) == 0
                             else np.asarray(fill, dtype=dtype))
    return v, v.ctypes.data_as(C.c_void_p), count


def _call(lib, entry, handle, obj, a):
    """-> status, and what the call gave besides it (None: nothing)"""
    from emagls_amd import _lib as L
    if entry in ("push_sets", "group_push"):
        d = obj or dict(nch=4, listeners=3, nmics=0)
        cols, n = d["nmics"] or d["nch"], max(a["nsamp"], 1)
        x, out = np.zeros((n, cols), order="F"), np.zeros((d["listeners"], 2, n))
        keep = [_array(a["set"], np.int32)] + [_array(a[k], np.float64) for k in ("yaw", "pitch", "roll")]
        args = [v for _, p, cnt in keep for v in (p, cnt)]
        f = lib.emagls_decode_group_push if entry == "group_push" else lib.emagls_decode_stream_push_sets
        return f(handle, None if a["null_in"] else x.ctypes.data_as(C.c_void_p), a["nsamp"], *args,
                 None if a["null_out"] else out.ctypes.data_as(C.c_void_p)), None
    if entry == "group_reset":
        return lib.emagls_decode_group_reset(handle, a["listener"]), None
    if entry in ("stream_info", "group_info"):
        v = [L.c_i64(-1) for _ in range(5 if entry == "group_info" else 4)] + [C.c_int(-1)]
        ptrs = [None] * len(v) if a["null_outs"] else [C.byref(x) for x in v]
        rc = (lib.emagls_decode_group_info if entry == "group_info" else lib.emagls_decode_stream_info)(handle, *ptrs)
        return rc, [x.value for x in v]
    if entry == "stream_sets":
        n = L.c_i64(-1)
        return lib.emagls_decode_stream_sets(handle, None if a["null_out"] else C.byref(n)), n.value
    if entry == "stream_destroy":
        return lib.emagls_decode_stream_destroy(handle), None
    if entry == "group_destroy":
        return lib.emagls_decode_group_destroy(handle), None
    raise KeyError(entry)


def _destroy(lib, kind, h):
    if h is not None and h.value:
        assert (lib.emagls_decode_group_destroy if kind == "group" else lib.emagls_decode_stream_destroy)(h) == 0


def _run(lib, objects, cases):
    """[status, message (None after a success, which leaves the last error alone), result] of every case"""
    from emagls_amd import _lib as L
    handles = {}
    try:
        for name, d in objects.items():
            entry = ("group_create" if d["kind"] == "group" else "create") + ("_encoded" if d["nmics"] else "" if d["kind"] == "group" else "_bank")
            a = dict(d, basis=REAL, in_c=0, null_wL=False, null_wR=False, null_out=False, null_enc=False)
            rc, handles[name], _ = _create(lib, entry, a)
            assert rc == L.OK and handles[name].value, (name, lib.emagls_last_error())
        got = []
        for entry, obj, a in cases:
            if "create" in entry:
                rc, h, left = _create(lib, entry, a)
                _destroy(lib, "group" if "group" in entry else "stream", h)
            else:
                rc, left = _call(lib, entry, handles[obj] if obj else None, objects.get(obj), a)
            got.append([rc, lib.emagls_last_error().decode() if rc else None, left])
        return got
    finally:
        for name, h in handles.items():
            _destroy(lib, objects[name]["kind"], h)


def record():
    """Writes the table with what the library in the tree answers.  To be run on the commit whose answers are the contract."""
    from emagls_amd import build, _lib
    build.build(jobs=4, verbose=False)
    cases = _table()
    got = _run(_lib.load(), OBJECTS, cases)
    assert all(g[0] in (0, 1, 2) for g in got), "a call of the table reached the device"
    rows = [dict(entry=e, object=o, arguments=a, status=g[0], message=g[1], result=g[2]) for (e, o, a), g in zip(cases, got)]
    with open(GOLDEN, "w") as f:
        f.write('{"objects": %s,\n "cases": [\n%s\n]}\n' % (json.dumps(OBJECTS), ",\n".join(json.dumps(r) for r in rows)))
    print("%d cases, %d of them errors, %d distinct messages" % (len(rows), sum(1 for r in rows if r["status"]),
                                                                 len({r["message"] for r in rows if r["status"]})))


@pytest.fixture(scope="module")
def lib():
    from emagls_amd import build, _lib
    build.build(jobs=4, verbose=False)
    return _lib.load()


def test_every_status_and_message_is_the_recorded_one(lib):
    with open(GOLDEN) as f:
        table = json.load(f)
    rows = table["cases"]
    assert [(r["entry"], r["object"]) for r in rows] == [(e, o) for e, o, _ in _table()]       # the recorded table is the whole one
    got = _run(lib, table["objects"], [(r["entry"], r["object"], r["arguments"]) for r in rows])
    wrong = [(r["entry"], r["object"], r["arguments"], [r["status"], r["message"], r["result"]], g)
             for r, g in zip(rows, got) if g != [r["status"], r["message"], r["result"]]]
    assert not wrong, "%d of %d calls answer differently; the first: %r" % (len(wrong), len(rows), wrong[:3])


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if os.environ.get("EMAGLS_RECORD_DECODE_PUSH_ERRORS") == "1":
        record()
    else:
        print(__doc__)
