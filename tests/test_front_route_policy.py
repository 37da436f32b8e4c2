"""Which kernels sample and score a forward call (esac_amd/csrc/front_route_policy.hpp: front_takes_route) through a stand-alone
host program -- tests/native/front_route_probe.cpp, built with the host compiler under AddressSanitizer and UBSan, its own
process, no GPU.  The route kernels have the headline call's modes compiled in and hold at most 8 cells per lane of the scorer,
so the predicate must be true for that call and false for every single deviation from it."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "front_route_probe.cpp")
EXE = os.path.join(HERE, "native", "front_route_probe_san")
DEPS = [SRC] + [os.path.join(HERE, "..", "esac_amd", "csrc", h) for h in ("front_route_policy.hpp", "sample_plan.hpp", "call_policy.hpp")] + \
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


# the headline call (bench.py, cfg2): esac.forward's default flags, one frame, 256 hypotheses, one expert, 60x80
CALL_ORDER = ("enabled", "serial", "caller_flags", "frames", "N", "E", "H", "W", "max_tries", "first_try", "hyp_offset", "cams", "shapes",
              "pack_flag", "hyp_index", "spec_flag", "tstamps", "errs")
HEADLINE = dict(enabled=1, serial=1, caller_flags=AUTO_EXACT, frames=1, N=256, E=1, H=60, W=80, max_tries=0, first_try=0, hyp_offset=0, cams=0,
                shapes=0, pack_flag=0, hyp_index=0, spec_flag=0, tstamps=0, errs=0)
RAW_ORDER = ("enabled", "serial", "frames", "N", "E", "H", "W", "flags", "max_tries", "first_try", "hyp_offset", "cams", "shapes", "packed",
             "hyp_index", "spec_flag", "tstamps", "errs")
RAW_HEADLINE = dict(enabled=1, serial=1, frames=1, N=256, E=1, H=60, W=80, flags=AUTO_EXACT | EXACT_SCORES | EXACT_SAMPLING, max_tries=1000000,
                    first_try=0, hyp_offset=0, cams=0, shapes=0, packed=0, hyp_index=0, spec_flag=0, tstamps=0, errs=0)


def _call(**kw):
    v = dict(HEADLINE, **kw)
    return "call " + " ".join(str(v[k]) for k in CALL_ORDER)


def _raw(**kw):
    v = dict(RAW_HEADLINE, **kw)
    return "raw " + " ".join(str(v[k]) for k in RAW_ORDER)


def test_the_headline_call_takes_the_route_kernels(probe):
    (kind, flags, max_tries, packed, route), = probe([_call()])
    assert kind == "call"
    assert int(flags) == AUTO_EXACT | EXACT_SCORES | EXACT_SAMPLING  # ESAC_FLAG_AUTO_EXACT applies: 256 * 60 * 80 <= 2^21
    assert int(max_tries) > 1024 and (int(packed), int(route)) == (0, 1)
    # ... and so do the other shapes and budgets the route kernels serve
    rows = probe([_call(N=1), _call(N=5), _call(H=13, W=17), _call(H=33, W=32), _call(H=64, W=128), _call(max_tries=3), _call(max_tries=200),
                  _call(caller_flags=EXACT_SCORES | EXACT_SAMPLING), _call(caller_flags=EXACT_SCORES), _call(caller_flags=EXACT_SCORES, H=1, W=1)])
    assert [int(r[4]) for r in rows] == [1] * len(rows), rows


CALL_DEVIATIONS = [
    dict(enabled=0),                                    # the switch off
    dict(serial=0),                                     # the speculative route
    dict(frames=2),                                     # a batch (ESAC_FLAG_AUTO_EXACT does not apply to batches)
    dict(frames=2, caller_flags=EXACT_SCORES),          # ... and with exact scores asked for
    dict(E=2),                                          # two experts: ESAC_FLAG_AUTO_EXACT does not apply
    dict(E=2, caller_flags=EXACT_SCORES | EXACT_SAMPLING),
    dict(N=257),                                        # ESAC_FLAG_AUTO_EXACT still applies; the sampler's plan is another kernel
    dict(N=257, caller_flags=EXACT_SCORES),
    dict(caller_flags=0),                               # fp32 scores: k_score_fast reads the fp32 rows
    dict(caller_flags=EXACT_SAMPLING),
    dict(caller_flags=STRICT),                          # strict reference: its own sampler and scorer
    dict(caller_flags=AUTO_EXACT | STRICT),
    dict(H=64, W=129),                                  # 256 * 64 * 129 > 2^21: ESAC_FLAG_AUTO_EXACT does not apply
    dict(H=64, W=129, caller_flags=EXACT_SCORES),       # exact scores asked for, but 8256 cells are more than 8 per lane
    dict(N=16, H=96, W=128),                            # ESAC_FLAG_AUTO_EXACT applies (16 * 12288 <= 2^21): 12 cells per lane
    dict(first_try=32),
    dict(hyp_offset=256),                               # a shard of a larger call
    dict(hyp_index=1),
    dict(cams=1),                                       # a camera table
    dict(cams=1, shapes=1),                             # a ragged table
    dict(pack_flag=1),                                  # ESAC_FLAG_PACK_MAPS: packed maps
    dict(spec_flag=1),
    dict(tstamps=1),
    dict(errs=1),                                       # ESAC_DEBUG_ERROR_IMAGE
]


@pytest.mark.parametrize("dev", CALL_DEVIATIONS, ids=[",".join("%s=%s" % kv for kv in d.items()) for d in CALL_DEVIATIONS])
def test_every_single_deviation_keeps_the_general_kernels(probe, dev):
    (kind, _flags, _tries, _packed, route), = probe([_call(**dev)])
    assert kind == "call" and int(route) == 0


def test_each_clause_of_the_predicate_alone(probe):
    """The predicate with every field as given: each clause refuses on its own, whatever the host would have derived."""
    assert probe([_raw()]) == [["raw", "1"]]
    off = [dict(enabled=0), dict(serial=0), dict(frames=2), dict(frames=0), dict(N=257), dict(N=0), dict(E=2), dict(E=0), dict(H=64, W=129),
           dict(H=8193, W=1), dict(H=0), dict(W=0), dict(H=65536, W=65536), dict(flags=AUTO_EXACT | EXACT_SAMPLING),
           dict(flags=RAW_HEADLINE["flags"] | STRICT), dict(first_try=1), dict(hyp_offset=1), dict(cams=1), dict(shapes=1), dict(shapes=2),
           dict(packed=1), dict(hyp_index=1), dict(spec_flag=1), dict(tstamps=1), dict(errs=1)]
    rows = probe([_raw(**d) for d in off])
    assert [r[1] for r in rows] == ["0"] * len(off), list(zip(off, rows))
    on = [dict(N=1), dict(H=64, W=128), dict(H=8192, W=1), dict(H=1, W=1), dict(flags=EXACT_SCORES), dict(max_tries=1), dict(max_tries=129)]
    rows = probe([_raw(**d) for d in on])
    assert [r[1] for r in rows] == ["1"] * len(on), list(zip(on, rows))
