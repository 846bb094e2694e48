"""gyre_amd/text_adapters.py against the REFERENCE's own functions.

tests/golden/ref_text_adapters_probe.py imports gyre/pipeline/textual_inversion.py, lora.py (its un-vendored lora_diffusion import
stubbed) and lycoris.py from /root/reference and EXECUTES apply_ti_to_tokenizer, apply_ti_to_encoder, match_encoder_to_tokenizer,
apply_kohya_to_pipe / set_lora_scale and apply_lycoris / set_lycoris_scale over the tiny encoder and stub tokenizer of
tests/text_adapter_util.py, next to this package's functions: token ids and embedding rows must agree exactly, encoder outputs in
float64 to rel-L2 <= 1e-10 (the gate of tests/test_text_adapters_host.py).  Build container only; a reference module that cannot
be imported here skips its own cases with the reason, the rest stays."""
import json
import os
import subprocess
import sys

import pytest

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")
GATE = 1e-10
FORMS = {"lora": "gyre.pipeline.lora", "loha": "gyre.pipeline.lycoris", "lokr_lowrank": "gyre.pipeline.lycoris",
         "lokr_dense": "gyre.pipeline.lycoris", "full": "gyre.pipeline.lycoris"}


@pytest.fixture(scope="module")
def probe():
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "ref_text_adapters_probe.py")], env=env,
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    line = [l for l in r.stdout.splitlines() if "PROBE_JSON " in l]
    assert r.returncode == 0 and line, (r.stdout + r.stderr)[-3000:]
    return json.loads(line[0].split("PROBE_JSON ", 1)[1])


def _need(probe, module):
    err = probe.get("import_errors", {}).get(module)
    if err:
        pytest.skip(f"the reference's {module} cannot be imported here: {err}")


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_textual_inversion_matches_the_reference_functions(probe, dtype):
    _need(probe, "gyre.pipeline.textual_inversion")
    c = probe[f"ti_{dtype}"]
    assert c["flattened_keys_equal"] and c["flattened_values_equal"] and c["token_ids_equal"] and c["mappings_equal"], c
    assert c["len"] == [132, 132]
    assert c["prompt_ids_ref"] == c["prompt_ids_mine"] and c["prompt_ids_mine"][3:8] == [128, c["prompt_ids_mine"][4], 129, 130, 131]
    assert c["table_shape"] == [[132, 32]] * 2 and c["table_dtype"] == [f"torch.{dtype}"] * 2
    assert c["added_rows_equal"] and c["old_rows_equal"] and c["rows_are_the_vectors"] and c["encoded_equal"], c
    assert c["shrunk_shape"] == [[128, 32]] * 2 and c["shrunk_equal"]


@pytest.mark.parametrize("weights", ["default", "text_encoder", "star_last"])
@pytest.mark.parametrize("form", list(FORMS))
def test_merged_encoder_matches_the_reference_hooks(probe, form, weights):
    _need(probe, FORMS[form])
    c = probe[f"{form}_{weights}"]
    assert c["effect"] > 1e-3, "the file does not move the encoder"
    assert c["rel_l2"] <= GATE and c["restored"], c


@pytest.mark.parametrize("form", list(FORMS))
def test_unknown_key_raises_the_references_error(probe, form):
    _need(probe, FORMS[form])
    ref, mine = probe[f"{form}_unknown_key"]
    assert ref[0] == mine[0] == "RuntimeError" and "Couldn't find model for lora_te_text_model_encoder_layers_0_mlp_fc9" in ref[1]
    assert "Couldn't find model for lora_te_text_model_encoder_layers_0_mlp_fc9" in mine[1]
