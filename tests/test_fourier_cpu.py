"""The sine first layer (Fourier features) on the host side: DNN's keywords and initialisation, the config keys, the
descriptor, old pickles, and the fp64 helper the GPU tests compare against.  No GPU needed."""
import io
import math
import pickle

import pytest
import torch
import torch.nn as nn

from pinn_depthestimation_amd import NetDesc
from pinn_depthestimation_amd._lib import ACT_LEAKY_RELU, ACT_SIN_TANH, ACT_TANH
from pinn_depthestimation_amd.config import load_config
from pinn_depthestimation_amd.dnn import DNN, Sin, activation_id_of, init_flat_params
from pinn_depthestimation_amd.engine import ACTIVATION_OF_INIT

from tests import fourier_util as F


def test_dnn_keywords_and_value_errors():
    m = DNN([3, 8, 8, 2], 0.0, "xavier")
    assert m.first_activation is None and m.fourier_sigma == 1.0 and m.activation_id == ACT_TANH
    assert isinstance(m.layers.activation_0, nn.Tanh)
    assert DNN([3, 8, 2], 0.0, "kaiming").activation_id == ACT_LEAKY_RELU
    s = DNN([3, 8, 8, 2], 0.0, "xavier", first_activation="sin", fourier_sigma=4.0)
    assert s.first_activation == "sin" and s.fourier_sigma == 4.0 and s.activation_id == ACT_SIN_TANH == 2
    assert isinstance(s.layers.activation_0, Sin) and isinstance(s.layers.activation_1, nn.Tanh)
    assert not list(Sin().parameters())
    assert list(s.state_dict()) == list(m.state_dict())               # the keys do not change
    assert isinstance(DNN([3, 8, 2], 0.0, "xavier", "sin").layers.activation_0, Sin)      # one hidden layer: the sine
    with pytest.raises(ValueError, match="xavier"):
        DNN([3, 8, 2], 0.0, "kaiming", first_activation="sin")
    with pytest.raises(ValueError, match="first_activation"):
        DNN([3, 8, 2], 0.0, "xavier", first_activation="cos")
    with pytest.raises(ValueError, match="fourier_sigma"):
        DNN([3, 8, 2], 0.0, "xavier", first_activation="sin", fourier_sigma=0.0)
    with pytest.raises(ValueError, match="xavier"):
        init_flat_params([3, 8, 2], "kaiming", first_activation="sin")
    assert activation_id_of("xavier") == ACT_TANH and activation_id_of("xavier", "sin") == ACT_SIN_TANH
    assert ACTIVATION_OF_INIT == {"xavier": ACT_TANH, "kaiming": ACT_LEAKY_RELU}          # stays a two-entry dict


def test_sin_module_on_the_cpu_is_the_fp64_helper():
    """The module tree itself (torch on the CPU) computes the helper's network."""
    torch.manual_seed(3)
    s = DNN([2, 5, 5, 3], 0.0, "xavier", first_activation="sin", fourier_sigma=2.0)
    X = F.points(7, 2, 1)
    params = [p.detach().clone() for p in s._ordered_params()]
    assert torch.allclose(s.layers(X), F.sin_mlp(params, X), rtol=0, atol=1e-6)


@pytest.mark.parametrize("sigma", [1.0, 4.0, 16.0])
def test_layer0_statistics(sigma):
    """The sample standard deviation of W_0 (64 x 3) over 50 seeds is within 10 % of sigma: of the 50 x 192 draws pooled (one
    seed's 192 draws scatter by sigma / sqrt(384) = 5 %, so a 10 % bar per seed would fail one seed in twenty by chance; each
    seed is held to 25 %, five of its standard deviations).  Phases inside [0, 2 pi); the other layers as before."""
    stds, others, pooled = [], [], []
    for seed in range(50):
        torch.manual_seed(seed)
        m = DNN([3, 64, 64, 4], 0.0, "xavier", first_activation="sin", fourier_sigma=sigma)
        W0, b0 = m.layers.layer_0.weight, m.layers.layer_0.bias.detach()
        assert W0.shape == (64, 3)
        stds.append(float(W0.detach().std()))
        pooled.append(W0.detach().reshape(-1).clone())
        assert float(b0.min()) >= 0.0 and float(b0.max()) < 2 * math.pi
        assert float(b0.max() - b0.min()) > math.pi                  # a spread of phases, not a constant
        # the other layers as before: Xavier-uniform weights inside their bound, zero hidden bias
        W1 = m.layers.layer_1.weight
        assert float(W1.abs().max()) <= math.sqrt(6.0 / 128) and float(m.layers.layer_1.bias.abs().max()) == 0.0
        assert float(m.layers.layer_2.weight.abs().max()) <= math.sqrt(6.0 / 68)
        flat = init_flat_params([3, 64, 64, 4], "xavier", torch.Generator().manual_seed(seed), first_activation="sin", fourier_sigma=sigma)
        others.append(float(flat[:192].std()))
        assert float(flat[192:256].min()) >= 0.0 and float(flat[192:256].max()) < 2 * math.pi
        assert float(flat[256 + 4096:256 + 4096 + 64].abs().max()) == 0.0
    for v in stds + others:
        assert abs(v - sigma) < 0.25 * sigma, (v, sigma)
    for v in (float(torch.cat(pooled).std()), float(torch.tensor(stds).pow(2).mean().sqrt()), float(torch.tensor(others).pow(2).mean().sqrt())):
        assert abs(v - sigma) < 0.10 * sigma, (v, sigma)
    assert abs(float(torch.cat(pooled).mean())) < 0.05 * sigma


def _parent_dnn_params(layers, init_type, seed):
    """The construction of the class as it was before it had the keywords, restated: nn.Linear's own draw, then the
    init_type's weight init, zero hidden bias."""
    torch.manual_seed(seed)
    out = []
    for i in range(len(layers) - 1):
        lin = nn.Linear(layers[i], layers[i + 1])
        if init_type == "kaiming":
            nn.init.kaiming_uniform_(lin.weight, nonlinearity="leaky_relu")
        else:
            nn.init.xavier_uniform_(lin.weight)
        if i < len(layers) - 2:
            nn.init.zeros_(lin.bias)
        out += [lin.weight.detach().clone(), lin.bias.detach().clone()]
    return out


def _parent_flat_params(layers, init_type, generator):
    parts = []
    n_lin = len(layers) - 1
    for i in range(n_lin):
        fan_in, fan_out = layers[i], layers[i + 1]
        bound = math.sqrt(6.0 / (fan_in + fan_out)) if init_type == "xavier" else math.sqrt(2.0) * math.sqrt(3.0 / fan_in)
        parts.append(torch.empty(fan_out * fan_in).uniform_(-bound, bound, generator=generator))
        if i < n_lin - 1:
            parts.append(torch.zeros(fan_out))
        else:
            b = 1.0 / math.sqrt(fan_in)
            parts.append(torch.empty(fan_out).uniform_(-b, b, generator=generator))
    return torch.cat(parts)


@pytest.mark.parametrize("init_type", ["xavier", "kaiming"])
def test_without_the_keyword_the_draws_are_bit_identical(init_type):
    layers = [3, 20, 20, 20, 4]
    for seed in (0, 1234):
        want = _parent_dnn_params(layers, init_type, seed)
        torch.manual_seed(seed)
        got = DNN(layers, 0.0, init_type)._ordered_params()
        torch.manual_seed(seed)
        got_kw = DNN(layers, 0.0, init_type, first_activation=None, fourier_sigma=9.0)._ordered_params()
        for w, g, gk in zip(want, got, got_kw):
            assert torch.equal(w, g.detach()) and torch.equal(w, gk.detach())
        a = init_flat_params(layers, init_type, torch.Generator().manual_seed(seed))
        b = init_flat_params(layers, init_type, torch.Generator().manual_seed(seed), first_activation=None, fourier_sigma=3.0)
        assert torch.equal(a, _parent_flat_params(layers, init_type, torch.Generator().manual_seed(seed))) and torch.equal(a, b)


def _raw(**layer_keys):
    return {"layers": dict({"input_features": 2, "hidden_layers": 3, "hidden_width": 20, "output_features": 6}, **layer_keys),
            "adam_optimizer": {"max_it": 1, "learning_rate": 1e-3}, "lbfgs_optimizer": {"max_it": 0},
            "loss": {"weight_fid_loss": 1, "weight_res_loss": 1},
            "data_fidelity": {"inputs": ["x", "y"], "outputs": ["h", "U"]},
            "data_residual": {"inputs": {k: {"requires_grad": ["true"]} for k in "xy"},
                              "outputs": ["h", "U", "V", "eta_mean", "Hrms", "k"]}}


def test_config_keys_absent_and_present():
    c = load_config(_raw())
    assert c.first_activation is None and c.fourier_sigma == 1.0
    c = load_config(_raw(first_activation="sin"))
    assert c.first_activation == "sin" and c.fourier_sigma == 1.0
    c = load_config(_raw(first_activation="sin", fourier_sigma=8))
    assert c.first_activation == "sin" and c.fourier_sigma == 8.0 and isinstance(c.fourier_sigma, float)
    with pytest.raises(ValueError, match="first_activation"):
        load_config(_raw(first_activation="relu"))


def test_trainer_and_tester_pass_the_keys_on():
    import numpy as np
    from pinn_depthestimation_amd.inference import Tester
    from pinn_depthestimation_amd.trainer import PINN
    cfg = load_config(_raw(first_activation="sin", fourier_sigma=4.0))
    Xr = np.random.RandomState(0).rand(32, 2).astype(np.float32)
    tr = PINN(None, None, Xr, cfg, device="cpu", checkpoint_every=0)
    assert tr.dnn.first_activation == "sin" and tr.dnn.fourier_sigma == 4.0 and tr.dnn.activation_id == ACT_SIN_TANH
    assert tr.evaluator.eng.desc.activation == ACT_SIN_TANH
    buf = io.BytesIO()
    torch.save(tr.dnn.state_dict(), buf)
    path = buf.getvalue()
    import os, tempfile
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "m.pth")
        open(f, "wb").write(path)
        t = Tester(f, cfg, device="cpu")
        assert t.model.activation_id == ACT_SIN_TANH and torch.equal(t.model.flat_params(), tr.dnn.flat_params().cpu())
    plain = PINN(None, None, Xr, load_config(_raw()), device="cpu", checkpoint_every=0)
    assert plain.dnn.activation_id == ACT_TANH and plain.evaluator.eng.desc.activation == ACT_TANH


def test_netdesc_carries_activation_2():
    d = NetDesc.from_layers([3, 64, 64, 4], (0, 1, 2), ACT_SIN_TANH)
    c = d.c_struct()
    assert c.activation == 2 and (c.d_in, c.d_out, c.n_hidden, c.width, c.k) == (3, 4, 2, 64, 3)
    assert d.with_(engine=4).c_struct().activation == 2


def test_pickles_without_the_new_attributes_still_load():
    torch.manual_seed(0)
    m = DNN([2, 6, 6, 3], 0.0, "xavier")
    m.__dict__.pop("first_activation"); m.__dict__.pop("fourier_sigma")     # the class as it was before the keywords
    old = pickle.loads(pickle.dumps(m))
    assert old.first_activation is None and old.fourier_sigma == 1.0 and old.activation_id == ACT_TANH
    for k in ("layer_sizes", "init_type", "dropout_rate", "_grad_cols_override", "first_activation", "fourier_sigma"):
        m.__dict__.pop(k, None)                                             # the reference's class: none of this module's attributes
    ref = pickle.loads(pickle.dumps(m))
    assert ref.layer_sizes == [2, 6, 6, 3] and ref.init_type == "xavier" and ref.first_activation is None
    assert ref.activation_id == ACT_TANH
    s = pickle.loads(pickle.dumps(DNN([2, 6, 6, 3], 0.0, "xavier", first_activation="sin", fourier_sigma=2.0)))
    assert s.first_activation == "sin" and s.fourier_sigma == 2.0 and s.activation_id == ACT_SIN_TANH
    assert isinstance(s.layers.activation_0, Sin)


def test_fp64_helper_against_a_hand_written_two_layer_formula():
    """y = W1 sin(W0 x + b0) + b1;  dy/dx_j = W1 (cos(W0 x + b0) * W0[:, j]);  and the gradient of a squared-output sum."""
    layers = [2, 5, 3]
    params = [q.double() for q in F.make_params(layers, 4.0, seed=2)]
    X = F.points(9, 2, 3).double()
    W0, b0, W1, b1 = params
    z = X @ W0.t() + b0
    Y = torch.sin(z) @ W1.t() + b1
    dY = torch.stack([(torch.cos(z) * W0[:, j]) @ W1.t() for j in range(2)])
    Yh, dYh = F.jet(params, X, (0, 1))
    assert torch.allclose(Yh, Y, rtol=0, atol=1e-14) and torch.allclose(dYh, dY, rtol=0, atol=1e-13)
    # gradient of sum(Y^2) w.r.t. W0 by hand: dL/dz = (2 Y W1) * cos z ; dL/dW0 = dL/dz^T X
    p = [q.clone().requires_grad_(True) for q in params]
    L = (F.sin_mlp(p, X) ** 2).sum()
    g = torch.autograd.grad(L, p)
    gz = (2 * Y @ W1) * torch.cos(z)
    assert torch.allclose(g[0], gz.t() @ X, rtol=0, atol=1e-12) and torch.allclose(g[1], gz.sum(0), rtol=0, atol=1e-12)
    # the three-hidden-layer form: sine first, tanh after
    params3 = [q.double() for q in F.make_params([2, 4, 4, 4, 1], 1.0, seed=5)]
    a = torch.sin(X @ params3[0].t() + params3[1])
    a = torch.tanh(a @ params3[2].t() + params3[3])
    a = torch.tanh(a @ params3[4].t() + params3[5])
    assert torch.allclose(F.sin_mlp(params3, X), a @ params3[6].t() + params3[7], rtol=0, atol=1e-14)
    assert float(params3[3].abs().min()) > 0 and float(params3[5].abs().min()) > 0        # non-zero hidden biases


def test_term_sums_and_yardstick_of_a_case():
    c = F.loss_case("pe", 2, 10, 17)
    ts64, _, g64 = c["ref"]
    ts32, _, g32 = c["y32"]
    assert ts64.shape == (3,) and g64.numel() == 2 * 10 + 10 + 10 * 10 + 10 + 10 * 6 + 6
    assert F.err(ts32, ts64) < 1e-4 and F.err(g32, g64) < 1e-4 and bool(torch.isfinite(g64).all())
    assert F.bar("sums", 0.0) == 2e-6 and F.bar("grad", 1e-5) == 4e-5
    b = F.blocks(c["layers"])
    assert b["W0"] == slice(0, 20) and b["b0"] == slice(20, 30) and b["blast"].stop == g64.numel()
