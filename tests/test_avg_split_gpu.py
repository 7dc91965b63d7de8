"""
GPU suite (`pytest -m gpu`) for the split CFR+ average pairs: the cases of avg_split_cases.py at the same sizes on the hipcc-built library -- the
pair kinds (D,U), (C,D), (D,C), (C,U), (U,C) of the board pass against the unpaired path, bit for bit.
"""
import pytest

import avg_split_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from pokerrl_amd import _native
    _native.require_device()
    lib = _native.lib()
    assert lib.prl_build_flavor() == b"hip-gfx950"
    return lib


@pytest.mark.parametrize("n,k", sc.CASE1)
def test_gpu_split_pairs_in_one_call_and_across_calls(L, monkeypatch, n, k):
    sc.case1(L, monkeypatch, n, k)


def test_gpu_split_pairs_start_at_the_first_blending_iteration(L, monkeypatch):
    sc.case2_delay(L, monkeypatch)


def test_gpu_generic_instantiation_takes_each_sets_kind(L, monkeypatch):
    sc.case3_no_steady(L, monkeypatch)


@pytest.mark.parametrize("key,kw", sc.CASE4, ids=[c[0] for c in sc.CASE4])
def test_gpu_split_pairs_on_the_other_registered_shapes(L, monkeypatch, key, kw):
    sc.case4_shape(L, monkeypatch, key, kw)


def test_gpu_split_pairs_with_several_boards_per_workgroup(L, monkeypatch):
    sc.case5_boards_per_workgroup(L, monkeypatch)


def test_gpu_split_pairs_on_weighted_boards(L, monkeypatch):
    sc.case6_weighted(L, monkeypatch)


@pytest.mark.parametrize("key,kw", sc.CASE7, ids=[c[0] for c in sc.CASE7])
def test_gpu_neither_pairs_nor_splits(L, monkeypatch, key, kw):
    sc.case7_not_taken(L, monkeypatch, key, kw)


def test_gpu_checkpoint_of_a_split_run(L, monkeypatch):
    sc.case8_checkpoint(L, monkeypatch)


def test_gpu_switch_restores_whole_board_pairs(L, monkeypatch):
    sc.case9_switch(L, monkeypatch)


def test_gpu_split_path_vs_oracle(L, monkeypatch):
    sc.case_oracle(L, monkeypatch)
