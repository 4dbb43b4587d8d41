"""The GEMM host dispatcher (csrc/kernels/gemm.hip: plan selection and plan validation) decides
exactly what tests/golden/gemm_plans.json records: the plan, workspace size and check codes of
every model shape at the bucket edges of the token count, under each environment switch, and
the check code of explicit plans (table plans, refused plans, plans with one field that has no
kernel) on both weight layouts and every epilogue. Runs on CPU: none of it launches.

The fixture is written by tools/dump_gemm_plans.py; each variant is re-derived in a fresh child
process, because the switches are parsed once per process."""
import importlib.util
import os

import pytest

from butterfly_amd import ops

pytestmark = pytest.mark.skipif(not ops.load_library(), reason="kernel library not built")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dump_gemm_plans", os.path.join(ROOT, "tools", "dump_gemm_plans.py"))
dump = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump)


@pytest.fixture(scope="module")
def golden():
    return dump.load_fixture()


def test_fixture_covers_every_variant(golden):
    assert sorted(golden) == sorted(dump.VARIANTS)
    assert len(golden["default"]["plan_checks"]) == 4 * len(dump.explicit_plans())
    codes = {c for row in golden["default"]["plan_checks"] for c in row[10:]}
    assert codes == {0, -1, -2, -4, -5}     # the grid reaches every answer the check can give


@pytest.mark.parametrize("variant", list(dump.VARIANTS))
def test_dispatcher_matches_the_recorded_decisions(golden, variant):
    got, want = dump.collect(variant), golden[variant]
    assert sorted(got) == sorted(want)
    for key in want:
        assert len(got[key]) == len(want[key]), (variant, key)
        for g, w in zip(got[key], want[key]):
            if key == "shapes":
                assert g[:3] == w[:3]
                assert len(g[3]) == len(w[3]) == len(dump.MS)
                for gr, wr in zip(g[3], w[3]):
                    assert gr == wr, (variant, "N, K, epi", g[:3], "got", gr, "recorded", wr)
            else:
                assert g == w, (variant, key, "got", g, "recorded", w)
