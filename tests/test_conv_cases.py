"""The case table of the convolution kernel tests (conv_cases.py) reaches what it claims: every case resolves,
through the planner of the built library (rf_conv_plan_query: host arithmetic, no GPU), to the (family, code) it
names, and the instantiations the cases launch cover the production kernels of tests/golden/conv_plan_parent.json."""
import os

import pytest

import conv_cases
from test_conv_plan import TABLE, _lib, kernel_name

# production instantiations no case launches, each with its reason (at most 2 of the 42)
EXCEPTED = {}


def _set_env(case, monkeypatch):
    for k in [k for k in os.environ if conv_cases.knobs().match(k)]:
        monkeypatch.delenv(k)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("case", conv_cases.CASES, ids=lambda c: c.id)
def test_case_plans_to_its_kernel(case, monkeypatch):
    lib = _lib()
    _set_env(case, monkeypatch)
    p = conv_cases.plan_of(case)
    if case.study and not lib.study_build():
        assert p.refuse and p.kernel == lib.CONVK[case.family], p  # the production build refuses, and says which
        return
    assert (p.kernel, p.code, p.refuse) == (lib.CONVK[case.family], case.code, 0), (case, p)


def test_cases_cover_every_production_kernel(monkeypatch):
    lib = _lib()
    reached = set()
    for case in conv_cases.CASES:
        if case.study:
            continue
        _set_env(case, monkeypatch)
        reached.add(kernel_name(conv_cases.plan_of(case), case.prec == "f16", case.kind != "deconv"))
    missing = set(TABLE["kernels"]) - reached - set(EXCEPTED)
    assert len(TABLE["kernels"]) == 42 and len(EXCEPTED) <= 2 and set(EXCEPTED) <= set(TABLE["kernels"])
    assert not missing, f"no case launches {sorted(missing)}"
    assert not (set(EXCEPTED) & reached), "an excepted kernel is reached after all: drop the exception"


def test_cases_are_small_and_avoid_the_once_per_process_knob():
    for c in conv_cases.CASES:
        assert "RF_CONV_SMALL" not in c.env, c.id
        ho = c.h * (c.k if c.kind == "deconv" else 1)
        wo = c.w * (c.k if c.kind == "deconv" else 1)
        assert c.n * ho * wo * c.cout <= (1 << 26) and (c.id == "phased-persistent" or c.n * c.h * c.w <= 8192), c.id
    assert sum(c.n >= 2 for c in conv_cases.CASES) >= len(conv_cases.CASES) - 3
