"""The cases of tests/test_gpu_headline_bits.py and of its fixture's generator (tests/golden/make_headline_bits.py): single calls of
the headline route -- k_sample<256, 2>, k_rescore, k_refine_team -- that take the paths a register or layout change in those
kernels can break without the default frames noticing: the sampler's second round (one try per lane), an exhausted try
budget, teams with one, two and three cells per lane.

Inputs: synthetic.make_frame(k, E=1, ...), RNG seed 1320, call k; the default score route, as tests/test_gpu_parity.py runs it."""
import numpy as np
import torch

from esac_amd import api
from esac_amd import synthetic as S

SEED = 1320

# name -> frame arguments, hypotheses, engine / oracle keywords, team size (None: the default policy)
CASES = {
    "second_round_k0": dict(k=0, frame=dict(outlier_frac=0.6), N=256),
    "second_round_k1": dict(k=1, frame=dict(outlier_frac=0.6), N=256),
    "second_round_k2": dict(k=2, frame=dict(outlier_frac=0.6), N=256),
    "exhausted_budget": dict(k=0, frame=dict(), N=256, kw=dict(max_tries=8)),
    "one_cell_per_lane": dict(k=0, frame=dict(H=32, W=40), N=7),              # 1280 cells: five members of 256
    "team_default": dict(k=0, frame=dict(), N=256),                            # 60x80: ten members, two cells per lane
    "team_of_eight": dict(k=0, frame=dict(), N=256, team=8),                   # 60x80: eight members, three cells per lane
}
# what a case's fixture holds, and the buffer it is read from
BUFFERS = {"tries": api.BUF_TRIES, "sample_xy": api.BUF_SAMPLE_XY, "hyps": api.BUF_HYPS, "scores": api.BUF_SCORES,
           "inlier_counts": api.BUF_INLIER_COUNTS, "inlier_map": api.BUF_INLIER_MAP}
RECORD_WORDS = 31  # the record up to (not including) its validity / epoch / status words, which count calls


def frame_of(case):
    c = CASES[case]
    f = S.make_frame(c["k"], E=1, **c["frame"])
    return f, S.gating_assignment(f, c["N"])


def run_device(engine, case):
    """One call of the case on the device: {name: array} of its outputs (the record's first RECORD_WORDS words as `record`)."""
    c = CASES[case]
    f, ha = frame_of(case)
    E, _, H, W = f["coords"].shape
    p = engine.make_params(E, H, W, len(ha), shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"],
                           sub_sampling=f["sub"], seed=SEED, call=c["k"], **c.get("kw", {}))
    if c.get("team") is not None:
        engine.set_refine_team(c["team"])
    try:
        res = engine.forward_device(torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda(), p)
        out = {name: np.array(engine.read(buf)) for name, buf in BUFFERS.items()}
        out["record"] = np.array(res[:RECORD_WORDS], dtype=np.float64)
        out["refine_info"] = engine.refine_info()
    finally:
        if c.get("team") is not None:
            engine.set_refine_team(api.REFINE_TEAM_DEFAULT)
    return out


def run_oracle(oracle, case):
    c = CASES[case]
    f, ha = frame_of(case)
    kw = c.get("kw", {})
    return oracle.forward(f["coords"], ha, shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"],
                          sub_sampling=f["sub"], seed=SEED, call=c["k"], max_tries=kw.get("max_tries", 0), max_ref_steps=kw.get("max_ref_steps", -1))


def bits(a):
    """float64 arrays as their bit patterns (NaN payloads and signed zeros count); integer arrays as they are."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a
