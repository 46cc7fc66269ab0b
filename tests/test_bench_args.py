"""bench.py's command line on the host: a plain run is the default, the other legs sit behind --full."""
import pytest

from bench import parse_args


def test_plain_run_is_the_default():
    a = parse_args(["--steps", "7", "--warmup", "2"])
    assert a.full is False and a.graph is False and a.steps == 7 and a.warmup == 2 and a.batch == 16


def test_graph_is_a_leg_of_full(capsys):
    a = parse_args(["--full", "--graph"])
    assert a.full is True and a.graph is True
    with pytest.raises(SystemExit) as e:
        parse_args(["--graph"])
    assert e.value.code == 2 and "--full" in capsys.readouterr().err
