"""The "sites" of tests/golden/skinny_forms.json are what the library launches.

The table holds the batch-row launches of the decode step, of the prologue's BiLSTM step and of the voice tower's LSTM step as integers - chunks per K segment,
tiles, epilogue, summed segment - and tests/test_skinny_form_host.py pins the kernel each of them takes.  Here l2s_op_step_site (libl2s_diag.so) runs the
builders of csrc/decode_step.h - the ones the decode loop, the training forward, the prologues, the voice tower and the chain microbenches call - on a finalised
model under the options each site stands for, and the groups that come out are compared with the table's, field for field.  Nothing of the step is launched;
the device is needed only to finalise the model (the suite's synthetic checkpoint plus synthetic voice-tower weights)."""
import pytest

from lip2speech_amd import statespec, synth
import parity_common as pc
import skinny_op_common as sk

pytestmark = pytest.mark.gpu

SITES = ("bilstm_step", "phase_a_unfolded", "phase_a_folded_step0", "phase_a_folded", "step_attention_proj", "phase_d_k1536", "phase_d_k1280",
         "phase_d_k1024_sum", "phase_d_k1024_unfolded", "phase_e", "step_fc_out_stop", "spk_lstm_step")


@pytest.fixture(scope="module")
def table():
    return sk.load_table()


@pytest.fixture(scope="module")
def nm(synth_sd):
    sd = dict(synth_sd)
    sd.update(synth.synth_state_dict(statespec.speaker_encoder_spec("speaker_encoder."), seed=99))
    return pc.fresh_native_model(sd, diag=True)


def test_the_list_is_the_tables(table):
    assert list(table["sites"]) == list(SITES) and table["group_fields"][:6] == ["nchunks0", "nchunks1", "nchunks2", "nchunks3", "ntiles", "epi"]


@pytest.mark.parametrize("site", SITES)
@pytest.mark.parametrize("rows", (3, 256))
def test_site_is_what_the_builders_launch(table, nm, site, rows):
    got = nm.step_site(site, rows)
    print(site, rows, got)
    assert [g[:6] + [g[7]] for g in got] == table["sites"][site]      # [nchunks x 4, ntiles, epi, a_sum set]; the groups do not depend on the rows
    # weight planes exist for LSTM groups only (planes_note); the folded LSTM0 matrices of K = 1536 / 1280 have none
    assert all(g[5] == sk.LSTM for g in got if g[6])
