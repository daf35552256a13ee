"""CPU tests of the evaluation driver (drl_graph_exploration_amd/evaluate.py): the CSV writer against a section of the
reference's own result file, its padding rule, and the table that maps the command line's (method, model) pairs onto the
network classes.  No engine is constructed."""
import os

import pytest


def _read_csv(path):
    """A file of the reference's format as write_csv's input: (records, category, map size).  The format does not mark where an
    episode was done: a row that repeats the row before it inside one decision is taken as the start of the padding (an executed
    action that left all three metrics unchanged would be indistinguishable from it - good enough for the fixture, whose padding
    is the 280 repeats of step 120's row; not a parser for the product, which has none)."""
    from drl_graph_exploration_amd import evaluate as E
    with open(path) as f:
        lines = f.read().split("\n")
    assert lines[0] == E.HEADER, "not an evaluation CSV: %r" % lines[0][:80]
    records, category, map_size = [], None, None
    rec, step = None, 0
    for ln in lines[1:]:
        if not ln:
            continue
        cat, t, ms, err, ent, unc, st = ln.split(",")
        category = cat
        if t:  # a decision
            map_size = float(ms)
            if rec is None or (rec["done"] and step >= E.PLOT_MAX_STEP[int(map_size)]):
                rec, step = dict(seed=len(records), done=False, stalled=False, decisions=[]), 0
                records.append(rec)
            rec["decisions"].append(dict(time=float(t), rows=[]))
            continue
        row = [float(err), float(ent), float(unc)]
        step = int(float(st))
        rows = rec["decisions"][-1]["rows"]
        if rec["done"] or (rows and rows[-1] == row):
            rec["done"] = True  # (padding: the reference repeats the last row only after `done`)
            continue
        rows.append(row)
    return records, category, int(map_size)


def test_write_csv_reproduces_the_reference_file_byte_for_byte(golden_dir, tmp_path):
    """tests/golden/eval_csv_seed0_DQN_GCN.csv = the header and seed 0's rows of the reference's data/test_result/40_DQN_GCN.csv
    (one episode, padded to step 400): parsed into records and written again, every byte must come back - row layout, the
    empty cells, the floats' shortest round-trip form, the steps and the map size as floats, the padding after done."""
    from drl_graph_exploration_amd import evaluate as E
    src = os.path.join(golden_dir, "eval_csv_seed0_DQN_GCN.csv")
    records, category, map_size = _read_csv(src)
    assert category == "DQN+GCN" and map_size == 40 and len(records) == 1
    rec = records[0]
    n_rows = sum(len(d["rows"]) for d in rec["decisions"])
    assert rec["done"] and 20 <= len(rec["decisions"]) and 90 <= n_rows < 400  # (the padding was recognised as padding)
    out = tmp_path / "40_DQN_GCN.csv"
    E.write_csv(records, str(out), category, map_size)
    want = open(src, "rb").read()
    got = out.read_bytes()
    assert got == want
    assert [p.name for p in tmp_path.iterdir()] == ["40_DQN_GCN.csv"]  # (the temporary file is gone)


def test_write_csv_pads_a_finished_episode_to_plot_max_step_and_no_further(tmp_path):
    from drl_graph_exploration_amd import evaluate as E
    rows = [[0.5, 130.25, 0.1], [0.25, 129.5, 0.2], [0.125, 128.0, 0.30000000000000004]]
    rec = dict(seed=0, done=True, stalled=False, decisions=[dict(time=0.001, rows=rows[:2]), dict(time=0.002, rows=rows[2:])])
    p = tmp_path / "a.csv"
    E.write_csv([rec], str(p), "A2C+g-U-Net", 40)
    lines = p.read_text().split("\n")
    assert lines[0] == E.HEADER and lines[-1] == ""
    body = lines[1:-1]
    steps = [ln for ln in body if not ln.split(",")[1]]
    assert len(body) == 2 + 400 and len(steps) == 400
    assert body[0] == "A2C+g-U-Net,0.001,40.0,,,," and body[3] == "A2C+g-U-Net,0.002,40.0,,,,"
    assert steps[0] == "A2C+g-U-Net,,,0.5,130.25,0.1,1.0"
    assert steps[2] == "A2C+g-U-Net,,,0.125,128.0,0.30000000000000004,3.0"
    for k in range(3, 400):  # the last 397 repeat row 3 with the step running on
        assert steps[k] == "A2C+g-U-Net,,,0.125,128.0,0.30000000000000004,%d.0" % (k + 1)
    # an episode that is not done (cut by max_decisions) is not padded; one that is longer than plot_max_step neither
    E.write_csv([dict(rec, done=False)], str(p), "A2C+g-U-Net", 40)
    assert len(p.read_text().split("\n")) == 1 + 2 + 3 + 1
    long = dict(seed=0, done=True, stalled=False, decisions=[dict(time=0.5, rows=[[1.0, 2.0, 3.0]] * 401)])
    E.write_csv([long], str(p), "DQN+GCN", 40)
    body = p.read_text().split("\n")[1:-1]
    assert len(body) == 1 + 401 and body[-1] == "DQN+GCN,,,1.0,2.0,3.0,401.0"
    # two seeds follow one another, each with its own step count; the larger maps pad further
    E.write_csv([rec, rec], str(p), "DQN+GCN", 60)
    body = p.read_text().split("\n")[1:-1]
    assert len(body) == 2 * (2 + 1200) and body[1202] == "DQN+GCN,0.001,60.0,,,," and body[-1].endswith(",1200.0")


def test_argument_table_resolves_every_method_and_model():
    from drl_graph_exploration_amd import evaluate as E
    from drl_graph_exploration_amd import networks as NW
    want = {("DQN", "GCN"): NW.GCN, ("DQN", "GG-NN"): NW.GGNN, ("DQN", "g-U-Net"): NW.GraphUNet,
            ("A2C", "GCN"): NW.PolicyGCN, ("A2C", "GG-NN"): NW.PolicyGGNN, ("A2C", "g-U-Net"): NW.PolicyGraphUNet}
    for (method, model), cls in want.items():
        got, args = E.model_spec(method, model)
        assert got is cls
        net = E.build_model(method, model)  # (host parameters only: no engine, no device)
        assert type(net) is cls
        if model == "g-U-Net":
            assert args == (5, 1000, 1000, 3)
            assert (net.in_channels, net.hidden_channels, net.out_channels, net.depth) == (5, 1000, 1000, 3)
        else:
            assert args == ()
    with pytest.raises(ValueError):
        E.model_spec("DQN", "MLP")
    with pytest.raises(ValueError):
        E.model_spec("PPO", "GCN")
    assert E.PLOT_MAX_STEP == {40: 400, 60: 1200, 80: 2400, 100: 4500}
    assert E.csv_path("out", 40, "A2C", "g-U-Net") == os.path.join("out", "40_A2C_g-U-Net.csv")
    assert E.default_weights("../data", "DQN", "GG-NN") == os.path.join("../data", "torch_weights", "DQN_GG-NN", "MyModel.pt")
    # the command line takes exactly these names
    with pytest.raises(SystemExit):
        E.main(["DQN", "MLP"])
