"""The attention kernels give the bits they gave before the host code around them was collapsed
into one entry pair with table-driven dispatch.

tests/golden/attention_parent_bits.json holds, per case of attention_oracle.PARENT_CASES, the
sha256 of the input bytes and of the o / lse / dq / dk / dv bytes, recorded on an MI355X from the
commit named in the file (`recorded_at_commit`, the parent of that change) with the ROCm version
named there, by `python tests/attention_oracle.py OUT.json COMMIT` run in a checkout of that
commit. The 17 cases reach every instantiation the dispatch tables launch at MODE 0: self,
grouped, cross and grouped cross attention, with and without dropout and the causal mask, and the
fused backward at its three lengths.

Re-recording is legitimate in two cases only: a change that alters the kernels' arithmetic on
purpose, and a compiler (ROCm) upgrade that alters their code. Record from the commit BEFORE the
change under test, never from the code under test, and let `recorded_at_commit` say which."""
import pytest

import attention_oracle as O


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(O.PARENT_CASES))
def test_attention_bits_equal_recorded_parent(cid):
    recorded = O.golden()["cases"][cid]
    inputs, sha = O.case_inputs(cid)
    assert sha == recorded["inputs"], "the input generator changed: these are not the recorded case's inputs"
    got = O.digests(O.run_wrappers(cid, inputs))
    assert got == {name: recorded[name] for name in O.OUTPUTS}


def test_recorded_cases_are_the_case_list():
    g = O.golden()
    assert list(g["cases"]) == list(O.PARENT_CASES) and len(g["cases"]) == 17
    assert len(g["recorded_at_commit"]) == 40 and g["rocm"]
