"""CPU characterisation of the training plumbing above the C ABI (ngf_amd._engine and the three modules on top of it): no GPU, no library call.

1. The three autograd nodes (train._TrainRender, infoinv_train._InfoInvRender, uv_train._UvRender) on CPU tensors against a stub engine: which
   engine a backward uses, when it renders its batch again, what it refuses, which gradients it asks for.
2. The get-or-grow rule of the models' engine attribute.
3. The bookkeeping of TrainerBase: step counters, ``frozen``, ``state_from``, the learning-rate decay."""
import types

import pytest
import torch

import ngf_amd  # noqa: F401
from ngf_amd import _lib, infoinv_train, train, uv_train

N, R, S = 2, 3, 4


class StubEngine:
    """What the nodes use of an engine: ``params``, ``_h``, ``forward(...) -> (..., ticket)``, ``backward(ticket, ..., want)``.  A ticket is live
    until the next forward; ``stale_answers`` more backwards answer "stale" whatever their ticket."""
    dev = torch.device("cpu")

    def __init__(self, params, outputs):
        self.params, self._h, self.outputs = list(params), 1, outputs
        self.forwards, self.backwards, self.ticket, self.stale_answers, self.wants = 0, 0, 0, 0, []

    def forward(self, *args):
        self.forwards += 1
        self.ticket += 1
        return (*self.outputs(*args), self.ticket)

    def backward(self, ticket, *rest):
        self.wants.append(list(rest[-1]))
        if ticket != self.ticket or self.stale_answers > 0:
            self.stale_answers = max(0, self.stale_answers - 1)
            return None
        self.backwards += 1
        return [torch.full_like(p, float(k + 1)) if w else None for k, (p, w) in enumerate(zip(self.params, rest[-1]))]


def _field_outputs(rays, jitter, S_, white, flag):
    return rays[:, :3].clone(), rays[:, 0].clone()


def _uv_outputs(cam, rd, bg, U):
    n, r, s = U.shape
    return torch.zeros(n, r, 3), torch.zeros(n, r), torch.zeros(n, r, s, 2), torch.zeros(n, r, s), torch.zeros(n, r, s, 3)


class Case:
    """One model: its node, the attribute its engine lives in, its getter and a forward through the node."""

    def __init__(self, name, flag=True, bg=True):
        self.name = name
        fn, self.attr, getter, nparams, outputs = {
            "triplane": (train._TrainRender, "_grad_engine", "_render_grad_engine", 15, _field_outputs),
            "infoinv": (infoinv_train._InfoInvRender, "_ii_engine", "_infoinv_grad_engine", infoinv_train.NPARAMS, _field_outputs),
            "uv": (uv_train._UvRender, "_uv_engine", "_uv_grad_engine", uv_train.NPARAMS, _uv_outputs)}[name]
        self.fn, self.outputs = fn, outputs
        self.params = [torch.ones(2, 2, requires_grad=(k != 1)) for k in range(nparams)]
        self.model = types.SimpleNamespace()
        self.asked = []                                   # the getter's calls: (rays, samples)
        self.engine = self.install(self.new_engine())

        def get(n, S_):
            self.asked.append((int(n), int(S_)))
            return getattr(self.model, self.attr)
        setattr(self.model, getter, get)
        if name == "uv":
            self.inputs = (torch.zeros(N, 3), torch.zeros(N, R, 3), torch.zeros(N, 3) if bg else None, torch.zeros(N, R, S))
        else:
            self.inputs = (torch.arange(12.).reshape(2, 6), torch.zeros(2), S, True, flag)

    def new_engine(self):
        return StubEngine(self.params, self.outputs)

    def install(self, eng):
        setattr(self.model, self.attr, eng)
        return eng

    def forward(self):
        return self.fn.apply(self.model, getattr(self.model, self.attr), *self.inputs, *self.params)

    def loss(self, out):
        return sum(o.sum() for o in out[:-1])           # the last output (depth / ray_pos) is not differentiable

    def grads(self):
        return [p.grad for p in self.params]


MODELS = ["triplane", "infoinv", "uv"]


@pytest.mark.parametrize("name", MODELS)
def test_a_backward_on_the_live_ticket_calls_backward_once_and_no_forward(name):
    c = Case(name)
    out = c.forward()
    assert len(out) == (5 if name == "uv" else 2) and not out[-1].requires_grad and all(o.requires_grad for o in out[:-1])
    c.loss(out).backward()
    e = c.engine
    assert (e.forwards, e.backwards, len(e.wants)) == (1, 1, 1) and c.asked == []
    for k, g in enumerate(c.grads()):
        if k == 1:
            assert g is None
        else:
            assert torch.equal(g, torch.full((2, 2), float(k + 1)))


@pytest.mark.parametrize("name", MODELS)
def test_a_stale_ticket_gives_one_more_forward_then_one_backward(name):
    c = Case(name)
    first = c.forward()
    c.forward()                                           # retires the first ticket
    c.loss(first).backward()
    e = c.engine
    assert (e.forwards, e.backwards, len(e.wants)) == (3, 1, 2) and c.asked == []
    assert torch.equal(c.params[0].grad, torch.full((2, 2), 1.0)) and c.params[1].grad is None


@pytest.mark.parametrize("name", MODELS)
def test_an_engine_replaced_on_the_model_takes_the_re_render_path_on_the_new_engine(name):
    c = Case(name)
    out = c.forward()
    old, new = c.engine, c.install(c.new_engine())
    c.loss(out).backward()
    assert (old.forwards, old.backwards, old.wants) == (1, 0, [])
    assert (new.forwards, new.backwards, len(new.wants)) == (1, 1, 1)
    assert c.asked == [(N * R if name == "uv" else 2, S)]
    assert torch.equal(c.params[2].grad, torch.full((2, 2), 3.0))


@pytest.mark.parametrize("name", MODELS)
def test_a_released_engine_is_replaced_through_the_getter(name):
    c = Case(name)
    out = c.forward()
    c.engine._h = None                                    # released, still in the attribute: the getter decides (here it returns the same object)
    c.loss(out).backward()
    assert len(c.asked) == 1 and (c.engine.forwards, c.engine.backwards) == (1, 1)


@pytest.mark.parametrize("name", MODELS)
def test_a_second_stale_answer_raises(name, monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: types.SimpleNamespace(ngf_last_error=lambda: b"the ticket is stale"))
    c = Case(name)
    out = c.forward()
    c.engine.stale_answers = 2
    with pytest.raises(RuntimeError, match="the ticket is stale"):
        c.loss(out).backward()
    assert (c.engine.forwards, c.engine.backwards, len(c.engine.wants)) == (2, 0, 2)


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("how", ["pointer", "shape"])
def test_a_re_allocated_parameter_tensor_is_refused(name, how):
    c = Case(name)
    out = c.forward()
    p = c.params[2]
    c.engine.params[2] = p.detach().clone() if how == "pointer" else p.detach()[:1]
    assert (c.engine.params[2].data_ptr() == p.data_ptr()) == (how == "shape")
    with pytest.raises(RuntimeError, match="re-allocated"):
        c.loss(out).backward()
    assert c.engine.backwards == 0 and c.engine.wants == []


@pytest.mark.parametrize("name", MODELS)
def test_want_follows_requires_grad(name):
    c = Case(name)
    for k in (0, 5, len(c.params) - 1):
        c.params[k].requires_grad_(False)
    c.loss(c.forward()).backward()
    off = {0, 1, 5, len(c.params) - 1}
    assert c.engine.wants == [[k not in off for k in range(len(c.params))]]
    assert all((g is None) == (k in off) for k, g in enumerate(c.grads()))


def test_triplane_with_the_gauge_off_asks_for_no_gauge_plane_gradients():
    c = Case("triplane", flag=False)
    c.loss(c.forward()).backward()
    assert c.engine.wants == [[k not in (1, 3, 4, 5) for k in range(15)]]
    assert all((g is None) == (k in (1, 3, 4, 5)) for k, g in enumerate(c.grads()))
    on = Case("infoinv", flag=False)                      # the InfoInv flag is a render mode, not a gauge: every gradient is asked for
    on.loss(on.forward()).backward()
    assert on.engine.wants == [[k != 1 for k in range(infoinv_train.NPARAMS)]]


def test_uv_without_a_background_and_with_unused_outputs():
    c = Case("uv", bg=False)
    seen = []
    backward = c.engine.backward
    c.engine.backward = lambda ticket, *rest: seen.append(rest[:-1]) or backward(ticket, *rest)
    color = c.forward()[0]
    (2.0 * color.sum()).backward()                        # transmittance, uv and the blend weight are not part of the loss
    (dc, dt, du, dw), = seen
    assert torch.equal(dc, torch.full((N, R, 3), 2.0)) and dc.dtype == torch.float32 and dc.is_contiguous()
    assert tuple(dt.shape) == (N, R) and not dt.any()
    assert (du is None or not du.any()) and (dw is None or not dw.any())
    assert (c.engine.forwards, c.engine.backwards) == (1, 1)


# --- the get-or-grow rule ---------------------------------------------------------------------------------------------------------------
class StubGrad:
    GROWS_FROM_RELEASED = True
    built = []

    def __init__(self, model, max_rays, max_samples):
        self.model, self.max_rays, self.max_samples, self._h, self.released = model, max_rays, max_samples, 1, 0
        StubGrad.built.append(self)

    def fits(self, n, S_, params):
        return n <= self.max_rays and S_ <= self.max_samples and params == "same"

    def release(self):
        self._h, self.released = None, self.released + 1


def test_get_or_grow_and_release():
    from ngf_amd import _engine
    m = types.SimpleNamespace()
    StubGrad.built = []
    a = _engine.grad_engine(m, "_eng", StubGrad, "same", 37, 8)
    assert m._eng is a and (a.max_rays, a.max_samples) == (37, 8)
    assert _engine.grad_engine(m, "_eng", StubGrad, "same", 37, 8) is a and _engine.grad_engine(m, "_eng", StubGrad, "same", 5, 3) is a
    b = _engine.grad_engine(m, "_eng", StubGrad, "same", 50, 4)             # too small: released, the successor has the larger of both shapes
    assert b is not a and m._eng is b and a.released == 1 and a._h is None and (b.max_rays, b.max_samples) == (50, 8)
    c = _engine.grad_engine(m, "_eng", StubGrad, "other", 1, 1)             # re-allocated parameters: a new engine as well
    assert c is not b and b.released == 1 and (c.max_rays, c.max_samples) == (50, 8)
    c.release()                                                             # released behind the model's back: rebuilt
    d = _engine.grad_engine(m, "_eng", StubGrad, "other", 1, 1)
    assert d is not c and d._h is not None and m._eng is d and len(StubGrad.built) == 4
    _engine.release_engine(m, "_eng")
    assert m._eng is None and d.released == 1 and d._h is None
    _engine.release_engine(m, "_eng")                                       # nothing to release: no error
    _engine.release_engine(types.SimpleNamespace(), "_eng")


def test_the_shape_of_a_released_engine_counts_where_the_engine_class_says_so():
    from ngf_amd import _engine
    assert train.RenderGrad.GROWS_FROM_RELEASED and infoinv_train.InfoInvGrad.GROWS_FROM_RELEASED and not uv_train.UvGrad.GROWS_FROM_RELEASED
    for keeps in (True, False):
        cls = type("G", (StubGrad,), {"GROWS_FROM_RELEASED": keeps})
        m = types.SimpleNamespace()
        _engine.grad_engine(m, "_eng", cls, "same", 50, 8).release()
        e = _engine.grad_engine(m, "_eng", cls, "same", 7, 2)
        assert (e.max_rays, e.max_samples) == ((50, 8) if keeps else (7, 2))


# --- TrainerBase bookkeeping ------------------------------------------------------------------------------------------------------------
def _trainer(shapes=((2, 2), (3,), (4,)), frozen=(), state_from=None, lr=(0.02, 1e-3, 1e-3)):
    from ngf_amd import _engine

    class T(_engine.TrainerBase):
        NAMES = ("plane", "dec.weight", "dec.bias")

        def optimizer_step(self):                         # a subclass's optimizer_step without its device call
            self.last = self._advance()
            self._decay()

    f = types.SimpleNamespace(device="cpu", nSamples=11)
    return T(f, [torch.zeros(s) for s in shapes], list(lr), batch_size=8, max_samples=None, lr_decay_iters=-1, lr_decay_target_ratio=0.1,
             n_iters=100, L1_reg_weight=8e-5, betas=(0.9, 0.99), eps=1e-8, frozen=frozen, state_from=state_from)


def test_frozen_parameters_keep_their_step_counters_and_frozen_takes_names_and_indices():
    t = _trainer(frozen=("dec.weight",))
    assert t.frozen == {1} and _trainer(frozen=(2, "plane")).frozen == {0, 2} and _trainer().frozen == set()
    assert t.max_samples == 11 and t.batch_size == 8 and tuple(t._loss.shape) == (2,) and t._loss.dtype == torch.float64
    for _ in range(3):
        t.optimizer_step()
    counts, lrs, idx = t.last
    assert t.steps == [3, 0, 3] and list(counts) == [3, 0, 3] and idx == [0, 2]
    assert [e.shape for e in t.exp_avg] == [p.shape for p in t.params] == [e.shape for e in t.exp_avg_sq]


def test_lr_decays_by_lr_factor_once_per_optimizer_step():
    t = _trainer()
    assert t.lr_factor == pytest.approx(0.1 ** (1 / 100))
    t.optimizer_step()
    counts, lrs, idx = t.last
    assert list(lrs) == pytest.approx([0.02, 1e-3, 1e-3], rel=1e-6)          # this step ran at the undecayed rates
    t.optimizer_step()
    assert t.lr == pytest.approx([x * t.lr_factor ** 2 for x in (0.02, 1e-3, 1e-3)], rel=1e-12)
    assert list(t.last[1]) == pytest.approx([x * t.lr_factor for x in (0.02, 1e-3, 1e-3)], rel=1e-6)


def test_state_from_carries_moments_of_unchanged_shapes_and_the_learning_rates():
    a = _trainer()
    for k in range(3):
        a.exp_avg[k].fill_(k + 1.0)
        a.exp_avg_sq[k].fill_(k + 10.0)
    a.optimizer_step()
    a.optimizer_step()
    b = _trainer(shapes=((2, 2), (5,), (4,)), state_from=a, lr=(1.0, 1.0, 1.0))
    assert b.steps == [2, 0, 2] and b.lr == a.lr and b.lr is not a.lr
    assert torch.equal(b.exp_avg[0], a.exp_avg[0]) and torch.equal(b.exp_avg_sq[2], a.exp_avg_sq[2]) and b.exp_avg[0] is not a.exp_avg[0]
    assert not b.exp_avg[1].any() and not b.exp_avg_sq[1].any() and b.exp_avg[1].shape == (5,)
