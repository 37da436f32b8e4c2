"""Which kernel a single frame's refinement team runs (esac_amd/csrc/refine_route_policy.hpp: refine_takes_route, and the fold
mode it depends on) through a stand-alone host program -- tests/native/refine_route_probe.cpp, built with the host compiler under
AddressSanitizer and UBSan, its own process, no GPU.  The route kernel has the headline call's modes compiled in, so the
predicate must be true for that call and false for every single deviation from it."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "refine_route_probe.cpp")
EXE = os.path.join(HERE, "native", "refine_route_probe_san")
DEPS = [SRC] + [os.path.join(HERE, "..", "esac_amd", "csrc", h) for h in ("refine_route_policy.hpp", "call_policy.hpp")] + \
    [os.path.join(HERE, "..", "include", "esac_hip.h")]

AUTO_EXACT, EXACT_SCORES, EXACT_SAMPLING, STRICT = 64, 1, 16, 256


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", SRC, "-o", EXE])

    def run(lines):
        out = subprocess.run([EXE], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
        rows = [l.split("|") for l in out.stdout.splitlines()]
        assert len(rows) == len(lines), out.stdout
        return rows
    return run


# the headline call (bench.py, cfg2): esac.forward's default flags, one frame, ten members, 256 hypotheses, one expert, 60x80
HEADLINE = dict(enabled=1, fold_enabled=1, caller_flags=AUTO_EXACT, frames=1, members=10, N=256, E=1, H=60, W=80, spec_mode=0, spec_gate=0,
                spec_debug=0, coop_extra=0, errs=0, tstamps=0)
CALL_ORDER = ("enabled", "fold_enabled", "caller_flags", "frames", "members", "N", "E", "H", "W", "spec_mode", "spec_gate", "spec_debug",
              "coop_extra", "errs", "tstamps")
RAW_ORDER = ("enabled", "frames", "members", "N", "E", "flags", "fold_select", "spec_mode", "spec_gate", "spec_debug", "coop_extra", "errs", "tstamps")
RAW_HEADLINE = dict(enabled=1, frames=1, members=10, N=256, E=1, flags=AUTO_EXACT | EXACT_SCORES | EXACT_SAMPLING, fold_select=2, spec_mode=0,
                    spec_gate=0, spec_debug=0, coop_extra=0, errs=0, tstamps=0)


def _call(**kw):
    v = dict(HEADLINE, **kw)
    return "call " + " ".join(str(v[k]) for k in CALL_ORDER)


def _raw(**kw):
    v = dict(RAW_HEADLINE, **kw)
    return "raw " + " ".join(str(v[k]) for k in RAW_ORDER)


def test_the_headline_call_takes_the_route_kernel(probe):
    (kind, flags, fold, route), = probe([_call()])
    assert kind == "call"
    assert int(flags) == AUTO_EXACT | EXACT_SCORES | EXACT_SAMPLING  # ESAC_FLAG_AUTO_EXACT applies: 256 * 60 * 80 <= 2^21
    assert (int(fold), int(route)) == (2, 1)
    # ... and so do the other shapes the route kernel is instantiated for
    rows = probe([_call(N=1), _call(N=4), _call(members=8), _call(members=16), _call(members=2, H=32, W=32),
                  _call(caller_flags=EXACT_SCORES | EXACT_SAMPLING), _call(caller_flags=EXACT_SCORES)])
    assert [(int(r[2]), int(r[3])) for r in rows] == [(2, 1)] * 7, rows


# (what deviates from the headline call, the fold mode the host then derives -- None: the same 2)
CALL_DEVIATIONS = [
    (dict(N=257), 0),                       # more hypotheses than a member has threads: no folded selection at all
    (dict(E=2), 1),                         # two experts: ESAC_FLAG_AUTO_EXACT does not apply -> the fp32 route's fold
    (dict(E=2, caller_flags=EXACT_SCORES | EXACT_SAMPLING), None),  # ... and with exact scores asked for: fold 2, but two experts
    (dict(caller_flags=0), 1),              # exact_scores off
    (dict(caller_flags=AUTO_EXACT, N=512, H=96, W=128), 0),  # ESAC_FLAG_AUTO_EXACT asked for where it does not apply, N > 256
    (dict(spec_mode=2), None),              # a speculative call's first refinement
    (dict(spec_gate=1), None),              # ... and its gated second one
    (dict(members=17), None),               # 17+ members: the LDS-staged exchange is the general kernel's
    (dict(members=32), None),
    (dict(members=0), 0),                   # no team
    (dict(caller_flags=STRICT), 0),         # strict-reference (implies exact scores; its statistics are k_stats_strict's)
    (dict(coop_extra=1), None),             # ESAC_DEBUG_COOP_STALL
    (dict(spec_debug=1), None),             # ESAC_DEBUG_SPEC_SECOND_BEST
    (dict(errs=1), None),                   # ESAC_DEBUG_ERROR_IMAGE
    (dict(tstamps=1), None),                # a timestamp buffer
    (dict(frames=2), 1),                    # a batch (ESAC_FLAG_AUTO_EXACT does not apply to batches)
    (dict(frames=2, caller_flags=EXACT_SCORES), None),
    (dict(fold_enabled=0), 0),              # ESAC_FOLD_SELECT=0
    (dict(enabled=0), None),                # the switch off
]


@pytest.mark.parametrize("dev,fold", CALL_DEVIATIONS, ids=[",".join("%s=%s" % kv for kv in d.items()) for d, _ in CALL_DEVIATIONS])
def test_every_single_deviation_keeps_the_general_kernel(probe, dev, fold):
    (kind, _flags, got_fold, route), = probe([_call(**dev)])
    assert kind == "call"
    assert int(got_fold) == (2 if fold is None else fold)
    assert int(route) == 0


def test_each_clause_of_the_predicate_alone(probe):
    """The predicate with every field as given: each clause refuses on its own, whatever the host would have derived."""
    assert probe([_raw()]) == [["raw", "1"]]
    off = [dict(enabled=0), dict(frames=2), dict(frames=0), dict(members=17), dict(members=1), dict(N=257), dict(E=2), dict(fold_select=0),
           dict(fold_select=1), dict(flags=RAW_HEADLINE["flags"] | STRICT), dict(spec_mode=1), dict(spec_mode=2), dict(spec_gate=1),
           dict(spec_debug=1), dict(coop_extra=1), dict(errs=1), dict(tstamps=1)]
    rows = probe([_raw(**d) for d in off])
    assert [r[1] for r in rows] == ["0"] * len(off), list(zip(off, rows))
    on = [dict(members=2), dict(members=8), dict(members=16), dict(N=1), dict(flags=EXACT_SCORES)]
    rows = probe([_raw(**d) for d in on])
    assert [r[1] for r in rows] == ["1"] * len(on), list(zip(on, rows))
