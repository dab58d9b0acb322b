"""Where ``PLIP.encode_images`` enqueues the device-side steps of a batch: every resize on the engine and stream of the lane that
encodes its rows, directly in front of that encode (plip_amd/image_routes.py).  Nothing here is timed or provoked: the wrappers only
read which engine object and which stream each step was given."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SECOND_SIZE = 96          # image_size= of the second resolution (tiny_b6: 64 px tiles, 16 px patches)
RECORDED = ("resize_crop_u8", "resize_crop_ragged", "encode_image_u8", "encode_image")


def _ptr(x):
    return x.data_ptr() if torch.is_tensor(x) else None          # (the ragged resize takes a list of host images)


@pytest.fixture
def recorded(monkeypatch):
    """The four entries wrapped on the ``Engine`` CLASS (clones and derived engines included): (name, id(engine), stream the call was
    made on, data_ptr of the tensor input, data_ptr of the result) per call."""
    from plip_amd.engine import Engine
    calls = []

    def wrap(name):
        inner = getattr(Engine, name)

        def method(self, x, *args, **kw):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            out = inner(self, x, *args, **kw)
            calls.append((name, id(self), stream, _ptr(x), _ptr(out)))
            return out
        return method

    for name in RECORDED:
        monkeypatch.setattr(Engine, name, wrap(name))
    return calls


@pytest.fixture(scope="module")
def inputs():
    rs = np.random.RandomState(31)
    same = [rs.randint(0, 256, size=(64 + 9, 64 + 4, 3), dtype=np.uint8) for _ in range(20)]
    differing = [rs.randint(0, 256, size=(40 + 7 * (i % 5) + i, 150 - 9 * (i % 4) - i, 3), dtype=np.uint8) for i in range(20)]
    assert len({im.shape for im in differing}) == 20
    return {"one size": same, "one size, CUDA tensor": np.stack(same), "differing sizes": differing}


# (the device tensor: at the second resolution, where the caller's tiles are cut at another size than the model takes)
@pytest.mark.parametrize("form,image_size", [("one size", None), ("one size", SECOND_SIZE), ("one size, CUDA tensor", SECOND_SIZE),
                                             ("differing sizes", None), ("differing sizes", SECOND_SIZE)])
def test_every_resize_runs_in_the_lane_that_encodes_its_rows(engines, recorded, inputs, form, image_size):
    """20 images in caller batches of 4 (max_batch 8): (1) every resize is directly followed by an encode_image_u8 on the same engine
    object and stream that reads the resize's output; (2) at least two (engine, stream) pairs occur, i.e. the lanes were on; (3) the
    embeddings are the bits of the same call with the lanes off."""
    from plip_amd.plip import PLIP
    model, cfg, *_ = engines("tiny_b6", "f32", 8)
    assert cfg.image_size == 64
    images = torch.from_numpy(inputs[form]).to(model.engine.device) if form.endswith("tensor") else inputs[form]
    plip = PLIP(model=model, ragged_resize=form == "differing sizes")
    used = [model.engine] + ([] if image_size is None else [model.engine.at_resolution(image_size, image_size)])
    before = [e.use_lanes for e in used]
    assert all(before)
    try:
        got = plip.encode_images(images, batch_size=4, image_size=image_size)
        calls = list(recorded)
        for e in used:
            e.use_lanes = False
        one_lane = plip.encode_images(images, batch_size=4, image_size=image_size)
    finally:
        for e, was in zip(used, before):
            e.use_lanes = was
    resizes = [i for i, c in enumerate(calls) if c[0].startswith("resize")]
    assert len(resizes) >= 3 and {calls[i][0] for i in resizes} == {"resize_crop_ragged" if form == "differing sizes" else "resize_crop_u8"}
    for i in resizes:
        name, engine, stream, _, out = calls[i]
        assert i + 1 < len(calls), "a resize with no encode behind it"
        nxt = calls[i + 1]
        assert nxt[0] == "encode_image_u8", (i, calls)
        assert nxt[1:3] == (engine, stream), f"call {i}: {name} on {(engine, stream)}, its encode on {nxt[1:3]}"
        assert nxt[3] == out, f"call {i}: the encode behind {name} does not read its output"
    assert len({c[1:3] for c in calls}) >= 2, "the lanes were off: nothing was checked"
    assert got.shape == (20, cfg.projection_dim) and np.array_equal(got, one_lane)
