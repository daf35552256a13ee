"""CPU tests of the GG-NN modules (scripts/Networks.py:73-122): construction, `state_dict` layout and init without a GPU, the
reference's checkpoints' keys, and the trainers' model factory."""
import io
import math

import pytest
import torch

import ggnn_ref

KEYS = {
    "gconv1.weight": (3, 1000, 1000),
    "gconv1.rnn.weight_ih": (3000, 1000),
    "gconv1.rnn.weight_hh": (3000, 1000),
    "gconv1.rnn.bias_ih": (3000,),
    "gconv1.rnn.bias_hh": (3000,),
    "fully_con1.weight": None,  # (out, 1000)
    "fully_con1.bias": None,
}


@pytest.mark.parametrize("name,out_dim", [("GGNN", 1), ("PolicyGGNN", 1), ("ValueGGNN", 100)])
def test_modules_construct_on_the_cpu_with_the_reference_layout(name, out_dim):
    from drl_graph_exploration_amd import networks
    torch.manual_seed(0)
    m = getattr(networks, name)()
    sd = m.state_dict()
    assert list(sd.keys()) == list(KEYS.keys())
    for k, shape in KEYS.items():
        want = shape if shape is not None else ((out_dim, 1000) if k.endswith("weight") else (out_dim,))
        assert tuple(sd[k].shape) == want and sd[k].dtype == torch.float32, k
    # init: weight and the GRU cell uniform in +-1/sqrt(1000) (PyG's `uniform(size, tensor)`, torch's GRUCell.reset_parameters), and
    # actually spread over that range; Linear(1000, out): +-1/sqrt(1000) too
    bound = 1.0 / math.sqrt(1000.0)
    for k, v in sd.items():
        assert float(v.abs().max()) <= bound, k
        if v.numel() >= 1000:
            assert float(v.abs().max()) > 0.95 * bound and abs(float(v.mean())) < 0.1 * bound, k
    assert [tuple(p.shape) for p in m.trunk_parameters()] == [tuple(sd[k].shape) for k in KEYS]
    assert len(list(m.parameters())) == 7  # (FusedAdam's limit is eight tensors)


def test_a_plain_torch_checkpoint_loads_strictly():
    """A `state_dict` saved from a plain-torch module that holds a real GRUCell under `gconv1.rnn` (what the reference's
    Networks.GGNN saves through PyG's GatedGraphConv) loads into the HIP-backed classes with strict=True, and back."""
    from drl_graph_exploration_amd import networks
    torch.manual_seed(1)
    for cls, out_dim in ((networks.GGNN, 1), (networks.PolicyGGNN, 1), (networks.ValueGGNN, 100)):
        ref = ggnn_ref.RefGGNN(1000, 3, out_dim)
        buf = io.BytesIO()
        torch.save(ref.state_dict(), buf)
        buf.seek(0)
        m = cls()
        m.load_state_dict(torch.load(buf, map_location="cpu"), strict=True)
        for a, b in zip(m.trunk_parameters(), ref.trunk_parameters()):
            assert torch.equal(a, b)
        ref.load_state_dict(m.state_dict(), strict=True)


def test_there_is_no_cpu_fallback():
    from drl_graph_exploration_amd import networks
    from drl_graph_exploration_amd._lib import DrlgxError
    data = networks.GraphData(torch.zeros(2, 5), torch.tensor([[0], [1]]), torch.ones(1))
    with pytest.raises(DrlgxError):
        networks.GGNN()(data, 0.0)


def test_model_factory_knows_both_families_and_still_refuses_g_u_net():
    from drl_graph_exploration_amd import networks
    from drl_graph_exploration_amd.train import make_models, paths
    cpu = torch.device("cpu")
    q, tgt = make_models("DQN", "GG-NN", cpu)
    assert type(q) is networks.GGNN and type(tgt) is networks.GGNN and q is not tgt
    actor, critic = make_models("A2C", "GG-NN", cpu)
    assert type(actor) is networks.PolicyGGNN and type(critic) is networks.ValueGGNN
    assert type(make_models("DQN", "GCN", cpu)[0]) is networks.GCN
    assert paths("d", "DQN", "GG-NN")[0] == "DQN_GG-NN/" and paths("d", "A2C", "GG-NN")[0] == "A2C_GG-NN/"
    with pytest.raises(NotImplementedError) as err:
        make_models("DQN", "g-U-Net", cpu)
    assert "g-U-Net" in str(err.value) and "GG-NN /" not in str(err.value)


def test_restatement_aggregates_at_the_target_node():
    """The checker itself on a case small enough to do by hand: one layer, hidden 2, identity weight, edge 0 -> 1 with weight 3:
    only node 1 receives (3 x node 0's state), so its GRU input differs from zero and node 0's does not."""
    conv = ggnn_ref.GatedGraphConv(2, 1).double()
    with torch.no_grad():
        conv.weight[0] = torch.eye(2)
    x = torch.tensor([[1.0, 2.0], [5.0, 7.0]], dtype=torch.float64)
    h = conv(x, torch.tensor([[0], [1]]), torch.tensor([3.0], dtype=torch.float64))
    want0 = conv.rnn(torch.zeros(1, 2, dtype=torch.float64), x[0:1])
    want1 = conv.rnn(3.0 * x[0:1], x[1:2])
    assert torch.allclose(h[0:1], want0) and torch.allclose(h[1:2], want1)
