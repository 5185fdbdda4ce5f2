"""The thread's last-error string is ONE object for the whole library.  The C entry points live in several translation units
(capi.hip, jobs.hip, decode_api.hip), the string itself and its only writer in another (host_pools.hip); each entry maps its
exceptions to a status and leaves the message where emagls_last_error() -- defined in capi.hip -- reads it.  A copy of that
string per translation unit would still build, and every entry would still return the right status: only the message would be a
stale one, or empty.

Entries of each file, each failing at its argument check before anything touches a device, with the status and the full message
the library gave before its host code was split into files.  Through ctypes; no GPU."""
import ctypes as C
import threading

import pytest


def _capi(lib):        # capi.hip
    return lib.emagls_device_count(None)


def _jobs(lib):        # jobs.hip: FromAtf (kind 4) is no kind of an HRIR-set list; the pointers must not be null, and are not dereferenced before the kind is
    buf = (C.c_double * 4)()
    p = C.cast(buf, C.c_void_p)
    return lib.emagls_design_hrir_sets(4, p, p, 1, 1, 1, p, p, 0.042, p, p, 1, 1, 48000.0, 1, 0, p, p)


def _jobs_shard(lib):  # jobs.hip, another entry with another message
    return lib.emagls_jobs_shard(None, 0, 1, 16, None, None, None)


def _decode(lib):      # decode_api.hip
    from emagls_amd import _lib as L
    n = L.c_i64(-1)
    return lib.emagls_decode_stream_sets(None, C.byref(n))


# entry -> (call, status, message), as recorded on the commit before the split
CALLS = {
    "capi": (_capi, 1, "null pointer"),
    "jobs": (_jobs, 2, "HRIR-set job lists: LS, MagLS, MagLS-2D, eMagLS, eMagLS2, EMAinCH, EMAinSH"),
    "jobs_shard": (_jobs_shard, 1, "invalid argument"),
    "decode": (_decode, 1, "null decode stream"),
}
# every entry is followed by one of a different file at least once, in both directions
ORDER = ["capi", "jobs", "decode", "capi", "decode", "jobs_shard", "capi", "jobs_shard", "jobs", "decode", "jobs"]


@pytest.fixture(scope="module")
def lib():
    from emagls_amd import build, _lib
    build.build(jobs=4, verbose=False)
    return _lib.load()


def _fail(lib, name):
    call, status, message = CALLS[name]
    assert call(lib) == status, name
    assert lib.emagls_last_error().decode() == message, name


def test_messages_differ_between_the_files():
    assert len({m for _, _, m in CALLS.values()}) == len(CALLS)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_each_file_leaves_its_own_message(lib, name):
    other = "decode" if name != "decode" else "capi"
    _fail(lib, other)          # a previous message, of another file
    _fail(lib, name)


def test_an_entry_of_another_file_replaces_the_message(lib):
    for name in ORDER:
        _fail(lib, name)


def test_the_string_is_per_thread_and_one_per_thread(lib):
    _fail(lib, "jobs")
    seen = {}

    def worker():
        try:
            seen["fresh"] = lib.emagls_last_error().decode()     # a new thread starts with an empty string
            for name in ORDER:
                _fail(lib, name)
            _fail(lib, "decode")
            seen["ok"] = True
        except BaseException as e:   # (an assertion in a thread would otherwise only be printed)
            seen["error"] = e

    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert "error" not in seen, seen["error"]
    assert seen["fresh"] == "" and seen["ok"]
    assert lib.emagls_last_error().decode() == CALLS["jobs"][2]   # the main thread's string is untouched
