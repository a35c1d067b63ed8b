"""What `process_args` decides for every --score crossed with the switches a score may or may not support, frozen:
tests/golden/cli_decisions.json was recorded by tests/golden/make_cli_decisions.py at the commit before the scores moved into
the table of mcm_amd/scores.py, and every command line must still be refused with the same message, or accepted with the same
resolved T, refine_threshold, predict and log directory.  Also: the table and the choices of --score name the same scores."""
import contextlib
import io
import json
import os

SCORES = ["MCM", "energy", "max-logit", "entropy", "var", "maha", "knn", "neglabel", "GL-MCM", "vim"]
EXTRAS = [[], ["--predict"], ["--refine-threshold", "on"], ["--refine-threshold", "exact"], ["--refine-threshold", "off"],
          ["--ctx", "x.npy"], ["--ctx", "x.npy", "--templates", "t.txt"], ["--dtype", "fp16x2"], ["--dtype", "bf16"],
          ["--maha-fit", "device"]]
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli_decisions.json")


def command_lines():
    """Every --score with every extra; neglabel both with and without its word file."""
    for score in SCORES:
        for words in ([[], ["--neg-words", "words.txt"]] if score == "neglabel" else [[]]):
            for extra in EXTRAS:
                yield ["--in_dataset", "ImageNet10", "--score", score] + words + extra


def decisions(workdir):
    """[{argv, error} or {argv, T, refine_threshold, predict, log_directory}] of `command_lines()`, with `workdir` as the working
    directory (process_args creates the log directory; the template and word files are written there)."""
    import eval_ood_detection as cli

    here = os.getcwd()
    os.chdir(workdir)
    try:
        with open("t.txt", "w") as f:
            f.write("a photo of a {c}\nan image of a {c}\n")
        with open("words.txt", "w") as f:
            f.write("anvil\nbucket\n")
        out = []
        for argv in command_lines():
            err = io.StringIO()
            try:
                with contextlib.redirect_stderr(err):
                    a = cli.process_args(argv)
            except SystemExit as e:
                out.append({"argv": argv, "exit": e.code, "error": err.getvalue().split(": error: ", 1)[1].strip()})
            else:
                out.append({"argv": argv, "T": a.T, "refine_threshold": a.refine_threshold, "predict": a.predict,
                            "log_directory": a.log_directory})
        return out
    finally:
        os.chdir(here)


def test_every_command_line_is_decided_as_recorded(tmp_path):
    with open(FIXTURE) as f:
        want = json.load(f)
    got = decisions(tmp_path)
    assert [d["argv"] for d in got] == [d["argv"] for d in want]
    for g, w in zip(got, want):
        assert g == w, (g, w)
    assert sum("error" in d for d in want) >= 30 and sum("T" in d for d in want) >= 50   # (the table holds both kinds)


def test_the_table_and_the_choices_of_score_name_the_same_scores():
    import eval_ood_detection as cli
    from mcm_amd.scores import METHODS

    choices = next(a.choices for a in cli.parser()._actions if a.dest == "score")
    assert sorted(choices) == sorted(SCORES) and len(set(choices)) == len(choices)
    assert sorted(METHODS) == sorted(choices)                          # one record per choice, no record without one
    assert all(name == m.name for name, m in METHODS.items())
