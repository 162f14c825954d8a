"""The column-tile pipeline of the fused scorer dgrad (csrc/dm_fused.hip) after its loads moved in front of the products: every output of
the forms h2h, h2, p3 and b16 carries the BITS of the build before that change (tests/golden/dm_fused_parent_bits.npz, written by
scripts/make_dm_fused_parent_bits.py from that build), at cases that walk the pipeline through its states - one tile, two, an odd count,
sixteen, a position per wave, a position per workgroup, a single position, partial last workgroups.  Every call is made twice into NaN-filled
outputs and must repeat itself: a load that had not landed when it was used shows as a difference or as a NaN.  What stands behind the valid
rows of the inputs (NaN or zeros) must not reach a result."""
import functools
import json

import numpy as np
import pytest

from tests import dm_fused_schedule_cases as S

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _fixture():
    with np.load(S.FIXTURE) as f:
        return json.loads(str(f["digests"])), {k: f[k] for k in f.files if k.startswith("out/")}


@functools.lru_cache(maxsize=None)
def _run(gpu, form, case):
    """(the NaN-behind launch of every case is shared by the two tests)"""
    from chameleon_recsys_amd import _lib
    return S.run_form(gpu, _lib.load(), form, case)


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
@pytest.mark.parametrize("form", S.FORMS)
def test_dm_fused_bits_are_the_parent_builds(gpu, form, case):
    digests, stored = _fixture()
    cid = S.case_id(case)
    assert S.inputs_digest(S.inputs(*case)) == digests["inputs/" + cid], "this host generates other inputs than the fixture's: nothing to compare"
    out = _run(gpu, form, case)
    want = {k.split("/")[-1]: v for k, v in digests.items() if k.startswith("%s/%s/" % (form, cid))}
    assert sorted(want) == sorted(out)
    bad = [k for k in sorted(out) if S.digest(out[k]) != want[k]]
    where = {}
    if bad and case == S.STORED:
        for k in bad:
            ref = stored["out/%s/%s" % (form, k)]
            idx = np.argwhere(out[k] != ref)
            where[k] = (len(idx), idx[:4].tolist())
    assert not bad, ("outputs differ from the parent build's bits", form, cid, bad, where)


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
@pytest.mark.parametrize("form", S.FORMS)
def test_dm_fused_nothing_behind_the_valid_rows_reaches_a_result(gpu, form, case):
    from chameleon_recsys_amd import _lib
    nan_behind = _run(gpu, form, case)
    zero_behind = S.run_form(gpu, _lib.load(), form, case, fill=0.0)
    for k in nan_behind:
        assert np.array_equal(nan_behind[k], zero_behind[k]), (form, S.case_id(case), k)
