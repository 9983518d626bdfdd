"""``beam_reorder`` over int8 suffix caches on MI355X: the int8 planes and their fp32 scale planes of every layer are
re-parented in one launch, bit-equal to ``index_select`` below the length and untouched from it on."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU runner
    pytest.skip("needs a GPU", allow_module_level=True)

from penroz.ops import beam_search as bs

LAYERS, CAP = [(2, 64), (1, 256)], 70  # two layers with different (Hkv, D); CAP · 4 B is no multiple of 16


@pytest.mark.parametrize("kind", ["identity", "repeated"])
@pytest.mark.parametrize("n", [0, 37, CAP])  # 37 scales end inside a 16-B unit
@pytest.mark.parametrize("W", [2, 8])
def test_beam_reorder_q8_is_index_select(W, n, kind):
    g = torch.Generator("cuda").manual_seed(W + n)
    planes = [[torch.randint(-128, 128, (W, h, CAP, d), device="cuda", generator=g, dtype=torch.int8) for h, d in LAYERS]
              for _ in "kv"]
    scales = [[torch.rand(W, h, CAP, device="cuda", generator=g) for h, _ in LAYERS] for _ in "kv"]
    parent = list(range(W)) if kind == "identity" else [W - 1] + [max(r - 1, 0) for r in range(1, W)]  # 0 twice (W > 2), a swap
    sel = torch.tensor(parent, device="cuda")
    every = planes[0] + planes[1] + scales[0] + scales[1]
    want = [c.clone() for c in every]
    for c in want:
        c[:, :, :n] = c[:, :, :n].index_select(0, sel)
    table = bs.ReorderTable(*planes, *scales)
    table.apply(sel.int(), torch.tensor([n], dtype=torch.int32, device="cuda"))
    for c, w in zip(every, want):  # slots from n on are untouched; identity parents write nothing
        assert torch.equal(c, w)
