"""No GPU: the size queries of the weight images answer what they answered when tests/golden/pack_images.json was recorded, and
refuse an id that names no network."""
import pytest

from attentive_dfprior_amd import _lib
import pack_images_golden as G


@pytest.mark.parametrize('name', G.NETS)
def test_size_queries_answer_the_recorded_values(name):
    want = G.golden()['sizes'][name]
    assert len(want) == (4 if name == 'att' else 5)
    assert G.sizes(_lib.lib(), name) == want


def test_the_recorded_sizes_hold_the_abi_tests_flat_counts():
    sizes = G.golden()['sizes']
    assert [sizes[n]['flat_floats'] for n in G.NETS] == [15800, 20920, 15899, 33410]


@pytest.mark.parametrize('query', ['adfp_decoder_flat_floats', 'adfp_decoder_packed_floats', 'adfp_decoder_packed_h_words',
                                   'adfp_decoder_packed_ht_words', 'adfp_train_act_floats'])
def test_size_queries_refuse_an_unknown_decoder_kind(query):
    for kind in (-1, _lib.NET_ID['att'], 4, 1 << 20):
        assert getattr(_lib.lib(), query)(kind) < 0, (query, kind)
    assert all(getattr(_lib.lib(), query)(k) > 0 for k in _lib.DEC_KIND.values())
