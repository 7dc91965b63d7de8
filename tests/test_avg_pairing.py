"""
CPU suite for the paired CFR+ average updates (avg_pairing_cases.py): the kernel sources on the SIMT emulator, the paired path against the
unpaired one (PRL_FHP_NO_AVG_PAIR=1) bit for bit, and against the CPU oracle. The same cases run on the real build in test_avg_pairing_gpu.py.
"""
import os
import sys

import pytest

import avg_pairing_cases as ac

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))


@pytest.fixture(scope="module")
def L():
    import build_emu
    from pokerrl_amd import _native
    lib = _native.bind(build_emu.build())
    assert lib.prl_build_flavor().startswith(b"emu")
    return lib


@pytest.mark.parametrize("n,k", ac.CASE1)
def test_emu_pairs_from_iteration_1_and_across_calls(L, monkeypatch, n, k):
    ac.case1(L, monkeypatch, n, k)


def test_emu_pairs_start_at_the_first_blending_iteration(L, monkeypatch):
    ac.case2_delay(L, monkeypatch)


def test_emu_generic_instantiation_defers_and_catches_up(L, monkeypatch):
    ac.case3_no_steady(L, monkeypatch)


@pytest.mark.parametrize("key,kw", ac.CASE4, ids=[c[0] for c in ac.CASE4])
def test_emu_pairs_on_the_other_registered_shapes(L, monkeypatch, key, kw):
    ac.case4_shape(L, monkeypatch, key, kw)


def test_emu_pairs_with_several_boards_per_workgroup(L, monkeypatch):
    ac.case5_boards_per_workgroup(L, monkeypatch)


def test_emu_pairs_on_weighted_boards(L, monkeypatch):
    ac.case6_weighted(L, monkeypatch)


@pytest.mark.parametrize("key,kw", ac.CASE7, ids=[c[0] for c in ac.CASE7])
def test_emu_pairing_is_not_taken(L, monkeypatch, key, kw):
    ac.case7_not_taken(L, monkeypatch, key, kw)


def test_emu_checkpoint_of_a_paired_run(L, monkeypatch):
    ac.case8_checkpoint(L, monkeypatch)


@pytest.mark.parametrize("n_iters,delay", [(5, 0), (6, 1)])
def test_emu_paired_path_vs_oracle(L, monkeypatch, n_iters, delay):
    ac.case_oracle(L, monkeypatch, n_iters, delay)
