"""etude_amd.BeatAnalyzer against the reference's own output (tests/golden/tempo_cases.json, written by tests/golden/make_golden_tempo.py from the reference class):
integers and list lengths exact, floats within 1e-12 relative (same operations in the same order; the margin covers another numpy build)."""
import json

import pytest

from etude_amd import BeatAnalyzer, TinyREMITokenizer

REL = 1e-12


def _cases(golden_dir):
    return json.loads((golden_dir / "tempo_cases.json").read_text())


def _same(got, want, where):
    assert type(got) is type(want) or (isinstance(got, (int, float)) and isinstance(want, (int, float))), (where, type(got), type(want))
    if isinstance(want, list):
        assert len(got) == len(want), (where, len(got), len(want))
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, f"{where}[{i}]")
    elif isinstance(want, dict):
        assert list(got) == list(want), where
        for k in want:
            _same(got[k], want[k], f"{where}.{k}")
    elif isinstance(want, int):
        assert isinstance(got, int) and got == want, where
    else:
        assert abs(got - want) <= REL * abs(want), (where, got, want)


def test_golden_covers_the_listed_behaviours(golden_dir):
    cases = _cases(golden_dir)
    assert len(cases) >= 12
    by = {c["name"]: c["output"] for c in cases}
    assert by["steady_3_4"][0]["time_sig"] == 3 and by["two_beats_per_bar_reads_as_4"][0]["time_sig"] == 4
    assert by["no_downbeats"] == [] and by["fewer_than_4_measures"] == []
    assert any(r["time_sig"] == 2 for r in by["hole_of_2_measures_filled_with_a_half_measure"])
    assert len(by["tempo_change"]) >= 2
    assert (golden_dir / "tempo_cases.json").stat().st_size < 256 * 1024


def test_analyze_data_matches_the_reference(golden_dir):
    for c in _cases(golden_dir):
        got = json.loads(json.dumps(BeatAnalyzer().analyze_data(c["input"])))
        _same(got, c["output"], c["name"])


def test_analyze_file_and_save_load_into_the_tokenizer(golden_dir, tmp_path):
    for c in _cases(golden_dir):
        p = tmp_path / "beat_pred.json"
        p.write_text(json.dumps(c["input"]))
        an = BeatAnalyzer()
        tempo = an.analyze(p)
        _same(json.loads(json.dumps(tempo)), c["output"], c["name"])
        out = tmp_path / "deep" / c["name"] / "tempo.json"
        an.save_tempo_data(tempo, out)
        assert json.loads(out.read_text()) == json.loads(json.dumps(tempo))
        if tempo:
            tk = TinyREMITokenizer(out)
            assert len(tk.tempo_data) == len(tempo)
