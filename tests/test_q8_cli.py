"""The engine CLI on llama2.c version-2 (Q8_0) checkpoints: fused and chained text against the Q8 reference loop
(tests/q8_ref.py) with a synthetic tokenizer at -r 0; the paths a Q8 model does not take exit with status 2."""
import os
import subprocess

import pytest

from oracle.tokenizer import Tokenizer, decode
from tests import q8_ref as R
from tests.helpers import GOLDEN
from tests.test_tokenizer_cli import ENGINE, cli_vocab, write_tokenizer

FIXTURES = ["ckpt_v2_q80_tied", "ckpt_v2_q80_untied"]


def run_engine(name, tokp, env_extra, prompt="hi b", steps=12):
    env = dict(os.environ, **env_extra)
    return subprocess.run([str(ENGINE), "-m", str(GOLDEN / f"{name}.bin"), "-t", str(tokp), "-p", prompt, "-s", str(steps), "-r", "0"],
                          capture_output=True, text=True, env=env, timeout=120)


@pytest.mark.parametrize("env", [{"RAMA_PATH": "ops"}, {"RAMA_WORLD": "2", "RAMA_RANK": "0"}])
def test_cli_refuses_ops_and_pipeline_on_q8(tmp_path, env):
    """refused before any GPU is touched"""
    tokp = tmp_path / "tok.bin"
    write_tokenizer(tokp, cli_vocab(64))
    r = run_engine("ckpt_v2_q80_tied", tokp, env)
    assert r.returncode == 2 and "Q8_0" in r.stderr, (r.returncode, r.stderr)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "chained"])
@pytest.mark.parametrize("name", FIXTURES)
def test_cli_q8_text_parity(tmp_path, name, path):
    import rama_amd
    cfg, gs, _, norms, t = R.read_v2(GOLDEN / f"{name}.bin")
    entries = cli_vocab(cfg["vocab_size"])
    assert len(entries) == cfg["vocab_size"]
    tokp = tmp_path / "tok.bin"
    write_tokenizer(tokp, entries)
    tok = Tokenizer(tokp, cfg["vocab_size"])
    prompt, steps = "hi b", 12
    dev = rama_amd.Hip(0)
    try:
        m = rama_amd.Q8Model.load(dev, GOLDEN / f"{name}.bin")
        rope = (m.tensor("freq_cis_real"), m.tensor("freq_cis_imag"))
        m.free()
    finally:
        dev.close()
    want_ids = R.Q8Ref(cfg, gs, norms, t, rope).generate(tok.encode(prompt), steps)
    r = run_engine(name, tokp, {"RAMA_PATH": path}, prompt, steps)
    if 0 in want_ids:                   # "<unk>" makes decode panic, as in the reference
        assert r.returncode == 101
        return
    assert r.returncode == 0, r.stderr
    body, _, tail = r.stdout.partition("\n--------------------------------\n")
    assert body == "".join(decode(tok.vocab[i]) for i in want_ids), (body, want_ids)
    assert tail.startswith("elapsed: ") and "avg tok/s: " in tail
