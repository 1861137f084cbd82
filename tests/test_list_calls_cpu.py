"""The argument checks of the fourteen list entry points without a GPU: tests/list_calls/host_list_calls.cpp on a host-only scene, host code
under ASan and UBSan, a program of its own (nothing is preloaded).  Every line it prints -- entry point, case, return code, xrt_last_error(),
what became of stats_out -- is the line of tests/golden/list_call_errors.txt, the recording made before the entry points shared their
helpers: the code and the wording of every check, which messages carry the function name, which family asks for the device first, what n == 0
does, that nothing is written without a device.  (The order among the checks of a family stays with the argument-order tests of its own module.)"""
import list_calls_py as lc


def test_every_call_answers_as_recorded():
    rc, lines, err = lc.run()
    assert rc == 0 and "runtime error" not in err and "Sanitizer" not in err, err[-4000:]
    want = lc.golden()
    for i, (got, exp) in enumerate(zip(lines, want)):
        assert got == exp, "line %d:\n  now:      %s\n  recorded: %s" % (i + 1, got, exp)
    assert len(lines) == len(want), (len(lines), len(want))


def test_the_recording_covers_every_entry_point():
    """What the comparison above is worth: every entry point has its lines, each with the valid call at n == 0 and n > 0, argument errors, and
    -- for the forms that look at their arguments before the device -- the host-only verdict; no line says an output was written."""
    want = [l.split(" | ") for l in lc.golden()]
    assert all(len(f) == 5 for f in want), [f for f in want if len(f) != 5][:3]
    for fn in lc.ENTRY_POINTS:
        mine = [f for f in want if f[0] == fn]
        cases = [f[1] for f in mine]
        assert len(mine) >= 12 and cases[0] == "valid, n == 0" and cases[1] == "valid, n > 0", (fn, len(mine))
        codes = {int(f[2]) for f in mine}
        assert -1 in codes and -3 in codes, (fn, codes)   # XRT_E_INVALID_ARG, XRT_E_NO_DEVICE
        assert any(f[1] == "null scene" and f[2] == "-1" and f[3] == fn + ": null scene" for f in mine), fn
        if fn.endswith("_device") and not fn.startswith("xrt_cast_rays"):   # (xrt_cast_rays[_paths]_device ask for the device before they look at alignment)
            assert any(f[3] == "device buffers must be 16-byte aligned" and f[2] == "-1" for f in mine), fn
    assert {f[0] for f in want} == set(lc.ENTRY_POINTS)
