"""The SVGP_FWD_SPLIT forms of the m <= 32 step in the plan (csrc/step_plan.hpp: StepPlan::fwd_split), read back as text.  The four
launch slots keep their names in svgp_mnist_step_route -- its text does not depend on the switch --, and svgp_mnist_step_route_forms
appends to each of them the entry the executor runs.  No GPU is needed: the plan is host arithmetic, and the four entries refuse a
configuration without the split before they touch a device."""
import ctypes as C
import os

import pytest

import svgp_vae_amd
from svgp_vae_amd import _lib

PHASE, STEP, DP = 0, 1, 2
SWITCHES = ["SVGP_DEC_SPLIT", "SVGP_ENC_KM_MERGE", "SVGP_SUM_MERGE", "SVGP_STAT_MERGE", "SVGP_AJI_DEC", "SVGP_DEC_FUSE", "SVGP_STAT_FOUR",
            "SVGP_KONLY_BRANCH", "SVGP_KBAR_BRANCH", "SVGP_SIDE_STREAMS", "SVGP_DP_PACK", "SVGP_FWD_SPLIT"]
# slot -> the entry that runs there with the split on
FORMS = {"svgp_gp_factor_fwd_defer_aji": "svgp_gp_factor_fwd_head", "svgp_gp_posterior_fwd": "svgp_gp_posterior_fwd_z",
         "svgp_mnist_decoder_fwd_bwd_data_pre_aji": "svgp_mnist_decoder_fwd_bwd_data_pre_tail",
         "svgp_gp_posterior_bwd_rows": "svgp_gp_posterior_bwd_rows_d"}
NEW = set(FORMS.values()) | {"svgp_gp_posterior_bwd_with_final_d"}


@pytest.fixture(scope="module", autouse=True)
def _library():
    if not os.path.exists(svgp_vae_amd.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def _text(monkeypatch, entry, form, phase=0, G=1, rank=0, adam=1, env=None, **cfg):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)
    kw = dict(b=64 if G == 1 else 32, b_global=64, m=32, L=16, M=8, n_obj=400, N_train=4050.0, jitter=1e-6)
    kw.update(cfg)
    buf = C.create_string_buffer(8192)
    _lib.call(entry, C.byref(_lib.MnistCfg(**kw)), form, phase, G, rank, adam, 0, buf, 8192)
    return buf.value.decode()


@pytest.mark.parametrize("form,G,m", [(STEP, 1, 32), (STEP, 1, 24), (DP, 2, 32)])
def test_the_route_text_does_not_depend_on_the_switch(monkeypatch, form, G, m):
    unset = _text(monkeypatch, "svgp_mnist_step_route", form, G=G, m=m)
    assert "svgp_gp_factor_fwd_defer_aji" in unset and not NEW & set(unset.split())
    for value in ("0", "1"):
        assert _text(monkeypatch, "svgp_mnist_step_route", form, G=G, m=m, env={"SVGP_FWD_SPLIT": value}) == unset


@pytest.mark.parametrize("L", [16, 57])
@pytest.mark.parametrize("adam", [1, 0])
@pytest.mark.parametrize("form,G", [(STEP, 1), (DP, 1), (DP, 3)])
def test_the_forms_printer_shows_exactly_the_four_new_forms(monkeypatch, form, G, adam, L):
    route = _text(monkeypatch, "svgp_mnist_step_route", form, G=G, adam=adam, L=L).splitlines()
    forms = _text(monkeypatch, "svgp_mnist_step_route_forms", form, G=G, adam=adam, L=L).splitlines()
    assert len(route) == len(forms)
    seen = []
    for plain, line in zip(route, forms):
        words = plain.split()
        if len(words) == 2 and words[1] in FORMS:
            assert line == f"{plain} -> {FORMS[words[1]]}"
            seen.append(words[1])
        else:
            assert line == plain
    assert seen == list(FORMS)                  # each slot once, in the step's order


def test_pass_two_kept_in_the_stage_takes_the_d_form_too(monkeypatch):
    for env in ({"SVGP_SUM_MERGE": "0"}, {"SVGP_ENC_KM_MERGE": "0"}):
        forms = _text(monkeypatch, "svgp_mnist_step_route_forms", STEP, env=env)
        assert "main svgp_gp_posterior_bwd_with_final -> svgp_gp_posterior_bwd_with_final_d\n" in forms
        assert "svgp_gp_posterior_bwd_rows" not in forms
    forms = _text(monkeypatch, "svgp_mnist_step_route_forms", DP, G=2, split_grad_exchange=1)
    assert "main svgp_gp_posterior_bwd_with_final -> svgp_gp_posterior_bwd_with_final_d\n" in forms


NONE = [dict(m=33), dict(m=64), dict(titsias=1)] + \
       [dict(env={name: "0"}) for name in ("SVGP_AJI_DEC", "SVGP_DEC_FUSE", "SVGP_DEC_SPLIT", "SVGP_FWD_SPLIT")]


@pytest.mark.parametrize("case", NONE, ids=str)
@pytest.mark.parametrize("form,G", [(STEP, 1), (DP, 2)])
def test_no_new_form_without_the_riders_in_the_fused_decoder_launch(monkeypatch, form, G, case):
    case = dict(case)
    env = case.pop("env", None)
    forms = _text(monkeypatch, "svgp_mnist_step_route_forms", form, G=G, env=env, **case)
    assert forms == _text(monkeypatch, "svgp_mnist_step_route", form, G=G, env=env, **case)
    assert "->" not in forms and not NEW & set(forms.split())


@pytest.mark.parametrize("phase", range(6))
def test_a_stand_alone_phase_keeps_the_full_forms(monkeypatch, phase):
    forms = _text(monkeypatch, "svgp_mnist_step_route_forms", PHASE, phase=phase)
    assert forms == _text(monkeypatch, "svgp_mnist_step_route", PHASE, phase=phase)
    assert "->" not in forms


def test_the_sharded_data_parallel_step_keeps_the_full_forms(monkeypatch):
    forms = _text(monkeypatch, "svgp_mnist_step_route_forms", DP, G=2, m=256)
    assert "reduce_scatter" in forms and "->" not in forms
    assert forms == _text(monkeypatch, "svgp_mnist_step_route", DP, G=2, m=256)


ENTRIES = [("svgp_gp_factor_fwd_head", (None, None)), ("svgp_gp_posterior_fwd_z", (None, None, None, None)),
           ("svgp_mnist_decoder_fwd_bwd_data_pre_tail", (None, None, None, None, None)),
           ("svgp_gp_posterior_bwd_rows_d", (None, None, None))]


@pytest.mark.parametrize("entry,rest", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_the_new_entries_refuse_what_has_no_split(entry, rest):
    """m > 32 and cfg.titsias are refused by the entry itself, with its own message, before any pointer is looked at or anything is
    launched (the device pointers here are NULL)."""
    kw = dict(b=64, b_global=64, L=16, M=8, n_obj=400, N_train=4050.0, jitter=1e-6)
    for m in (33, 64, 256):
        with pytest.raises(svgp_vae_amd.SvgpError, match=f"SVGP_FWD_SPLIT.*m <= 32, m = {m}"):
            _lib.call(entry, C.byref(_lib.MnistCfg(m=m, **kw)), *rest)
    with pytest.raises(svgp_vae_amd.SvgpError, match="SVGP_FWD_SPLIT.*titsias"):
        _lib.call(entry, C.byref(_lib.MnistCfg(m=32, titsias=1, **kw)), *rest)
