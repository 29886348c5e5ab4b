"""The kernels each configuration of the single-domain substep launches, and how often, against the record tests/golden/launch_census.json
(tests/launch_census.py: the table of cases and how the record is made).  A change of a route decision in tlab_amd/csrc/rhs.cpp shows here as another
census; a deliberate one re-records the file from the new code and says so."""
import json
import pytest
import launch_census as LC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_launch_census(name, monkeypatch):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    want = LC.recorded()[name]
    got = LC.census(name, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    if got != want:
        print("recorded:", json.dumps(want, sort_keys=True))
        print("launched:", json.dumps(got, sort_keys=True))
        print("differs: ", {t: (want.get(t), got.get(t)) for t in sorted(set(want) | set(got)) if want.get(t) != got.get(t)})
    assert got == want
