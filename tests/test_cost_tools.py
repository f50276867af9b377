"""tools/costlib.py and the eleven tools written against it, as far as they go without a device: every recorded summary under profiles/ is
reproduced by its tool's summarise(), the child runner stops at the first child that fails, every parser still has the options and defaults
it had before the tools shared a module, and the shared module pulls in neither torch nor the package."""
import importlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)

SIZES = dict(envs=4096, agents=2, steps=1000, warmup=64)
CHILDREN = dict(worker=None, parent_tree=None, repeats=3, child_timeout=150, out=None)
# {option: default} of every tool, from the add_argument lines the tools had when each carried its own parser
PARSERS = {
    "state_obs_cost": dict(SIZES, **CHILDREN, obs=0, configs="0,1"),
    "driver_cost": dict(SIZES, **CHILDREN, obs=0, configs="0,1"),
    "racecraft_cost": dict(SIZES, **CHILDREN, obs=0, configs="0,1"),
    "range_obs_cost": dict(SIZES, **CHILDREN, obs=0, state_obs=0, configs="0,1"),
    "grid_obs_cost": dict(SIZES, **CHILDREN, obs=0, others=0, stagger=1000, configs="0,1"),
    "contact_obs_cost": dict(SIZES, **CHILDREN, config="obs0", siblings=0, configs="obs0,obs1,drive"),
    "end_rules_cost": dict(SIZES, **dict(CHILDREN, child_timeout=240), config="obs0", siblings=0, patience=100, configs="obs0,obs1"),
    "level_pool_cost": dict(SIZES, **CHILDREN, stagger=1, levels=256, phases="1,0"),
    "level_stats_cost": dict(SIZES, **CHILDREN, stagger=1, obs=1, state_obs=0, levels=256, obs_settings="0,1"),
    "frame_skip_cost": dict(dict(SIZES, steps=2000), **CHILDREN, config="rgb", configs="rgb,gray4"),
    "obs_format_rate": dict(envs=4096, agents=2, steps=2000, warmup=200, stagger=1, legs="abcd"),
}


def _first_seen(runs, key):
    return list(dict.fromkeys(r[key] for r in runs))


# ---------------------------------------------------------------------------------------------- 1. recorded summaries reproduce
@pytest.mark.parametrize("name, by_config", [("state_obs", False), ("driver", False), ("racecraft", False), ("contact_obs", True),
                                             ("level_stats", False), ("end_rules", True)])
def test_recorded_summary_reproduces(name, by_config):
    tool = importlib.import_module(f"{name}_cost")
    with open(os.path.join(ROOT, "profiles", f"{name}_cost.json")) as f:
        rec = json.load(f)
    runs = rec["runs"]
    which = _first_seen(runs, "which")                       # (the children of a repeat are started in the order of the tool's `which`)
    assert which[0] == "parent"
    extra = (_first_seen(runs, "config"),) if by_config else ()
    assert json.dumps(tool.summarise(runs, which, *extra)) == json.dumps(rec["summary"])


def test_end_rules_recorded_verdict():
    import end_rules_cost
    with open(os.path.join(ROOT, "profiles", "end_rules_cost.json")) as f:
        rec = json.load(f)
    code, lines = end_rules_cost.verdict(rec["summary"], ["obs0", "obs1"])
    assert code == 2
    assert len(lines) == 2 and lines[0].startswith("FAIL obs0:") and lines[1].startswith("FAIL obs1:")
    assert end_rules_cost.verdict({}, ["obs0", "obs1"]) == (0, [])      # (no parent tree: no such key, nothing fails)


# ---------------------------------------------------------------------------------------------- 2. the runner stops at the first failure
CHILD = """import json, sys, time
log, mode, n = sys.argv[1:4]
with open(log, "a") as f:
    f.write(mode + " " + n + "\\n")
print("child output before the result", flush=True)
if mode == "exit3":
    print("the tail of the failing child")
    sys.exit(3)
if mode == "sleep":
    time.sleep(60)
if mode == "two":
    print("RESULT " + json.dumps(dict(n=-1)))
if mode != "silent":
    print("RESULT " + json.dumps(dict(n=int(n))))
"""


@pytest.fixture
def child(tmp_path):
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    log = tmp_path / "starts.log"

    def jobs(*modes):
        return [(f"{m} n={i}", [str(log), m, str(i)], 10 + i) for i, m in enumerate(modes)]

    def starts():
        return log.read_text().splitlines()
    return str(script), jobs, starts


def test_runner_runs_every_job_in_order(child, capsys):
    import costlib
    script, jobs, starts = child
    runs = costlib.run_children(script, jobs("ok", "two", "ok"), 30)
    assert runs == [dict(n=0, repeat=10), dict(n=1, repeat=11), dict(n=2, repeat=12)]      # the LAST `RESULT ` line of the second child
    assert starts() == ["ok 0", "two 1", "ok 2"]
    assert capsys.readouterr().out.splitlines() == [json.dumps(r) for r in runs]


@pytest.mark.parametrize("mode, code", [("exit3", 3), ("silent", 0), ("sleep", 124)])
def test_runner_stops_at_first_failure(child, capsys, mode, code):
    import costlib
    script, jobs, starts = child
    assert costlib.run_children(script, jobs("ok", mode, "ok"), 1 if mode == "sleep" else 30) is None
    assert starts() == ["ok 0", f"{mode} 1"]                 # two starts, not three
    out = capsys.readouterr().out
    assert "child output before the result" in out
    assert ("the tail of the failing child" in out) == (mode == "exit3")
    assert out.splitlines()[-1] == f"child {mode} n=1 ended with {code}: nothing more is started"


# ---------------------------------------------------------------------------------------------- 3. parsers are unchanged
@pytest.mark.parametrize("name", sorted(PARSERS))
def test_parser_options_and_defaults(name):
    tool = importlib.import_module(name)
    assert vars(tool.parser().parse_args([])) == PARSERS[name]


@pytest.mark.parametrize("name", sorted(PARSERS))
def test_help_needs_no_device(name):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    pr = subprocess.run([sys.executable, os.path.join(TOOLS, name + ".py"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert pr.returncode == 0, pr.stdout
    assert "--envs" in pr.stdout


# ---------------------------------------------------------------------------------------------- 4. the shared module imports clean
def test_costlib_imports_neither_torch_nor_the_package():
    code = "import sys; import costlib; print(sorted(m for m in ('torch', 'multi_car_racing_amd') if m in sys.modules))"
    pr = subprocess.run([sys.executable, "-c", code], cwd=TOOLS, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert pr.returncode == 0 and pr.stdout.strip() == "[]", pr.stdout
