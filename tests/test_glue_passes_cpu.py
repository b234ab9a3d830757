"""Host side of ``HipOps.fused_glue`` without a GPU: the encoder's CPU path takes a tuple of image tensors as their concatenation, and
a forward on a backend that is not the channels-last GPU path (the CPU oracle) never takes the position shortcut."""
import torch

from unimatch_amd import UniMatch
from unimatch_amd.encoder import CNNEncoder
from unimatch_amd.synth import CONFIGS, synth_images, synth_state_dict
from oracle import model as om
from tests.oracle_ops import OracleOps


def test_encoder_cpu_path_takes_a_tuple_as_the_concatenation():
    torch.manual_seed(3)
    for scales in (1, 2):
        enc = CNNEncoder(128, scales).eval()
        a, b = torch.randn(2, 3, 40, 56), torch.randn(1, 3, 40, 56)
        with torch.no_grad():
            want = enc(torch.cat([a, b], 0))
            got = enc((a, b))
            single = enc((a,))
        assert len(got) == len(want) == scales
        for g, w_ in zip(got, want):
            assert torch.equal(g, w_)
        assert torch.equal(single[0], enc(a)[0])


def test_forward_on_the_cpu_oracle_backend_never_takes_the_position_shortcut(monkeypatch):
    ck, fk = CONFIGS['gmflow_s1']
    model = UniMatch(**ck).eval()
    sd = synth_state_dict({k: v.shape for k, v in model.state_dict().items()})
    model.load_state_dict(sd)
    i0, i1 = synth_images(1, 64, 96, seed=1000, kind='shift')
    ops = OracleOps()
    ops.fused_glue = True                                        # even a backend that carries the knob: the path decides, not the knob
    seen = []
    encode, match = model._encode, model._match
    monkeypatch.setattr(model, '_encode', lambda images, task='flow', position=None: (seen.append(position), encode(images, task, position))[1])
    monkeypatch.setattr(model, '_match', lambda *a, **k: (seen.append(k.get('stream_has_pos')), match(*a, **k))[1])
    pred = model.bind_ops(ops)(i0, i1, **fk)['flow_preds'][0]
    assert seen == [None, False]
    want = om.unimatch_forward(sd, i0, i1, num_scales=1, upsample_factor=8, reg_refine=False, **fk)
    assert pred.shape == want.shape and (pred - want).abs().mean().item() < 1e-3
