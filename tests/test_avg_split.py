"""
CPU suite for the split CFR+ average pairs (avg_split_cases.py): the kernel sources on the SIMT emulator, the split path against the unpaired one
(PRL_FHP_NO_AVG_PAIR=1) bit for bit, and against the CPU oracle. The same cases run on the real build in test_avg_split_gpu.py.
"""
import os
import sys

import pytest

import avg_split_cases as sc

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))


@pytest.fixture(scope="module")
def L():
    import build_emu
    from pokerrl_amd import _native
    lib = _native.bind(build_emu.build())
    assert lib.prl_build_flavor().startswith(b"emu")
    return lib


def test_the_restated_schedule_runs_every_kind():
    sc.schedule_selfcheck()


@pytest.mark.parametrize("n,k", sc.CASE1)
def test_emu_split_pairs_in_one_call_and_across_calls(L, monkeypatch, n, k):
    sc.case1(L, monkeypatch, n, k)


def test_emu_split_pairs_start_at_the_first_blending_iteration(L, monkeypatch):
    sc.case2_delay(L, monkeypatch)


def test_emu_generic_instantiation_takes_each_sets_kind(L, monkeypatch):
    sc.case3_no_steady(L, monkeypatch)


@pytest.mark.parametrize("key,kw", sc.CASE4, ids=[c[0] for c in sc.CASE4])
def test_emu_split_pairs_on_the_other_registered_shapes(L, monkeypatch, key, kw):
    sc.case4_shape(L, monkeypatch, key, kw)


def test_emu_split_pairs_with_several_boards_per_workgroup(L, monkeypatch):
    sc.case5_boards_per_workgroup(L, monkeypatch)


def test_emu_split_pairs_on_weighted_boards(L, monkeypatch):
    sc.case6_weighted(L, monkeypatch)


@pytest.mark.parametrize("key,kw", sc.CASE7, ids=[c[0] for c in sc.CASE7])
def test_emu_neither_pairs_nor_splits(L, monkeypatch, key, kw):
    sc.case7_not_taken(L, monkeypatch, key, kw)


def test_emu_checkpoint_of_a_split_run(L, monkeypatch):
    sc.case8_checkpoint(L, monkeypatch)


def test_emu_switch_restores_whole_board_pairs(L, monkeypatch):
    sc.case9_switch(L, monkeypatch)


def test_emu_split_path_vs_oracle(L, monkeypatch):
    sc.case_oracle(L, monkeypatch)
