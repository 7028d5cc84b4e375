"""ComputeStereoMatches three ways on the CPU: the definition in plain numpy (oracle/stereo_definition.py)
against the C++ oracle on every planted case of tests/stereo_patterns.py and on one workload frame, uRight
and depth as bit patterns; every case's precondition (it reaches the branch it is named for, proved from
the definition's trace); the legal-key validator; and the coverage condition over the outcomes."""
import numpy as np
import pytest

import stereo_patterns as sp
from oracle import stereo_definition as sd

CASES = sp.all_cases() + sp.tall_cases() + sp.coarse_cases()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_geometry_matches_the_oracle(oracle_lib):
    """The float32 scale chain the cases are planted with is the oracle's; the capacity holds N = 1025."""
    for pair in ("tex", "coarse"):
        g = sp.PAIR_GEOM[pair]
        info = sp.oracles(pair, oracle_lib)[4]
        assert np.array_equal(_bits(info["scale"]), _bits(np.array(g.scale)))
        assert np.array_equal(_bits(info["inv_scale"]), _bits(np.array(g.inv)))
        pyr = sp.oracles(pair, oracle_lib)[2]
        assert [(p.shape[1], p.shape[0]) for p in pyr] == g.sizes
    for g in (sp.SMALL, sp.TALL, sp.COARSE):
        assert sp.capacity(oracle_lib, g) == sp.CAP[g] > 1100


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case(case, oracle_lib):
    """Legal keys, definition == oracle bit for bit, windows inside the kernel's load margins, and the
    precondition."""
    sp.validate(case, sp.CAP[case.g])
    ref = sp.reference(case, oracle_lib)
    our, odp, onm = ref["oracle"]
    dur, ddp, dnm, tr = ref["def"]
    assert dnm == onm == tr.n, f"{case.name}: {dnm} matches by the definition, {onm} by the oracle"
    assert np.array_equal(_bits(dur), _bits(our)), f"{case.name}: uRight differs at {np.nonzero(_bits(dur) != _bits(our))[0][:5]}"
    assert np.array_equal(_bits(ddp), _bits(odp)), f"{case.name}: depth differs at {np.nonzero(_bits(ddp) != _bits(odp))[0][:5]}"
    sp.check_windows(case, tr)
    case.pre(case, ref)


def test_outcomes_covered(oracle_lib):
    """Every outcome of the definition except `delta-out` (unreachable: DESIGN.md section 3) is reached by
    some case. A condition, not a measurement."""
    seen = set()
    for c in CASES:
        seen.update(sp.outcomes(sp.reference(c, oracle_lib)["def"][3]))
    assert seen == set(sd.OUTCOMES) - {"delta-out"}, f"missing {set(sd.OUTCOMES) - {'delta-out'} - seen}, extra {seen - set(sd.OUTCOMES)}"


def test_delta_stays_within_half(oracle_lib):
    """The argument for `delta-out` being dead, checked on every window search of every case: the winner is
    the first strict minimum, so d1 > d2 <= d3 and |deltaR| <= 0.5."""
    for c in CASES:
        for kt in sp.reference(c, oracle_lib)["def"][3].keys:
            if kt.delta is not None:
                d1, d2, d3 = kt.sads[5 + kt.bestinc - 1: 5 + kt.bestinc + 2]
                assert d1 > d2 <= d3 and abs(kt.delta) <= 0.5


def test_workload_frame(oracle_lib):
    """One 752 x 480 synthetic stereo frame at 1000 features, extracted by the oracle, through both."""
    from orb_slam3_ros_amd.synth import synth_stereo
    left, right = synth_stereo(500, 752, 480)
    ol = oracle_lib.OracleExtractor(1000, 1.2, 8, 20, 7)
    orr = oracle_lib.OracleExtractor(1000, 1.2, 8, 20, 7)
    _, kl, dl = ol(left)
    _, kr, dr = orr(right)
    bf, fx = 0.110078 * 458.654, 458.654
    our, odp, onm = oracle_lib.stereo_match(ol, orr, kl, dl, kr, dr, bf, fx)
    info = ol.level_info()
    pl = [ol.pyramid_level(l) for l in range(8)]
    pr = [orr.pyramid_level(l) for l in range(8)]
    dur, ddp, dnm, tr = sd.stereo_match(pl, pr, info["scale"], info["inv_scale"], kl, dl, kr, dr, bf, fx)
    ol.close()
    orr.close()
    assert dnm == onm
    assert np.array_equal(_bits(dur), _bits(our)) and np.array_equal(_bits(ddp), _bits(odp))
    assert int((our >= 0).sum()) > 300, f"{int((our >= 0).sum())} matches survive"
