"""
GPU suite (`pytest -m gpu`) for the paired CFR+ average updates: the cases of avg_pairing_cases.py that run kernels of their own, at the same
sizes, on the hipcc-built library -- the deferred / catch-up kinds of the board pass against the unpaired path, bit for bit.
"""
import pytest

import avg_pairing_cases as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from pokerrl_amd import _native
    _native.require_device()
    lib = _native.lib()
    assert lib.prl_build_flavor() == b"hip-gfx950"
    return lib


@pytest.mark.parametrize("n,k", ac.CASE1)
def test_gpu_pairs_from_iteration_1_and_across_calls(L, monkeypatch, n, k):
    ac.case1(L, monkeypatch, n, k)


def test_gpu_pairs_start_at_the_first_blending_iteration(L, monkeypatch):
    ac.case2_delay(L, monkeypatch)


def test_gpu_generic_instantiation_defers_and_catches_up(L, monkeypatch):
    ac.case3_no_steady(L, monkeypatch)


@pytest.mark.parametrize("key,kw", ac.CASE4, ids=[c[0] for c in ac.CASE4])
def test_gpu_pairs_on_the_other_registered_shapes(L, monkeypatch, key, kw):
    ac.case4_shape(L, monkeypatch, key, kw)


def test_gpu_pairs_with_several_boards_per_workgroup(L, monkeypatch):
    ac.case5_boards_per_workgroup(L, monkeypatch)


def test_gpu_paired_path_vs_oracle(L, monkeypatch):
    ac.case_oracle(L, monkeypatch, 5, 0)
