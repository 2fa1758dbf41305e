"""Every attribute of an engine exists from its constructor on: no pass, eval or training, adds one (several of them hold device
buffers that a captured graph keeps by address, so what an engine owns has to be readable in one place)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _resunet():
    from pssr2_amd.models import ResUNet
    return ResUNet(hidden=[16, 32], depth=1), (2, 1, 16, 16), 4


def _rdresunet():
    # the small configuration of test_gpu_rdmodel.test_bf16_vs_oracle (the reference fixtures' head width of 8 is below the 16 channels
    # that 16-bit storage needs)
    from pssr2_amd.models import RDResUNet
    kw = dict(channels=1, hidden=[64, 64, 64], scale=4, depth=1, rdnet_init=32, growth_rates=[16, 24, 32], ds_blocks=[False, True, True],
              ese_blocks=[False, True, True], n_blocks=[2, 2, 1])
    return RDResUNet(**kw), (2, 1, 48, 48), 4


@pytest.mark.parametrize("make", [_resunet, _rdresunet], ids=["resunet", "rdresunet"])
def test_engine_declares_all_state_up_front(make):
    torch.manual_seed(11)
    model, shape, scale = make()
    declared = set(vars(model._engine))
    model = model.cuda()
    model.compute_dtype = torch.bfloat16
    eng = model._engine
    x = torch.rand(*shape, device="cuda") * 255
    target = torch.rand(shape[0], 1, shape[2] * scale, shape[3] * scale, device="cuda")

    def eval_forward():
        model.eval()
        with torch.no_grad():
            model(x)

    eval_forward()
    model.train()
    for _ in range(2):
        torch.nn.functional.mse_loss(model(x) / 255, target).backward()
    eval_forward()
    torch.cuda.synchronize()
    now = set(vars(eng))
    assert now == declared, (sorted(now - declared), sorted(declared - now))

    # a pass that did not reach its end leaves entries in the work lists: reset_backward_state() empties every one of them
    model.train()
    model(x)
    assert eng.saved is not None
    for q in eng._QUEUES:
        getattr(eng, q).append(None)
    eng._deferred, eng._pending = (None, [], None), {0: None}
    eng.reset_backward_state()
    assert eng._QUEUES and all(getattr(eng, q) == [] for q in eng._QUEUES)
    assert eng.saved is None and eng._deferred is None and eng._pending == {} and not eng._side_on
    assert set(vars(eng)) == declared
