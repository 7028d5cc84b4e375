"""CPU side of tests/test_gpu_stereo_two_phase.py: every planted case is legal, the definition agrees with
the oracle bit for bit on it, its windows lie inside the kernel's load margins and its precondition
holds."""
import numpy as np
import pytest

import stereo_patterns as sp
import stereo_two_phase_patterns as tp

CASES = tp.all_cases()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case(case, oracle_lib):
    sp.validate(case, sp.CAP[case.g])
    ref = sp.reference(case, oracle_lib)
    our, odp, onm = ref["oracle"]
    dur, ddp, dnm, tr = ref["def"]
    assert dnm == onm == tr.n, f"{case.name}: {dnm} matches by the definition, {onm} by the oracle"
    assert np.array_equal(_bits(dur), _bits(our)) and np.array_equal(_bits(ddp), _bits(odp)), case.name
    sp.check_windows(case, tr)
    case.pre(case, ref)
