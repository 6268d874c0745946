"""The recorded weight images (tests/golden/pack_images.json): inputs, digests and the recorder.

The fixture holds names, sizes and SHA-256 digests only.  It was written by `python tests/pack_images_golden.py` on an MI355X from
the library's single-image C entries (adfp_pack_split_image with H | G, adfp_pack_decoder_ht / adfp_pack_attention_ht,
adfp_pack_decoder / adfp_pack_attention) as they stood BEFORE those entries became wrappers of the job kernel, so it anchors every
later route to images that no code of today produced.  Re-record only when a layout changes on purpose."""
import ctypes as C
import hashlib
import json
import os

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pack_images.json')
NETS = ('low', 'high', 'color', 'att')
FILL = 0x5A5A5A5A


def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def state_dicts():
    """name -> state dict: one with a weight the f16 split cannot hold (the attention network's range bit), one in range."""
    from oracle import adfp_oracle as O
    bad = O.random_state_dict(seed=9)
    bad['mlp.pts_linears.2.weight'][3, 5] = 9.0e4
    return {'seed9_out_of_range': bad, 'seed5': O.random_state_dict(seed=5)}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def sizes(L, name):
    """What the library's size queries answer for one network (no GPU needed)."""
    from attentive_dfprior_amd import _lib
    if name == 'att':
        return {'flat_floats': L.adfp_attention_flat_floats(), 'packed_floats': L.adfp_attention_packed_floats(),
                'packed_h_words': L.adfp_attention_packed_h_words(), 'packed_ht_words': L.adfp_attention_packed_ht_words()}
    k = _lib.DEC_KIND[name]
    return {'flat_floats': L.adfp_decoder_flat_floats(k), 'packed_floats': L.adfp_decoder_packed_floats(k),
            'packed_h_words': L.adfp_decoder_packed_h_words(k), 'packed_ht_words': L.adfp_decoder_packed_ht_words(k),
            'train_act_floats': L.adfp_train_act_floats(k)}


def filled(name, fmt, device):
    """A buffer for `name`'s image in format `fmt` ('h' / 'g' / 'hg' share one), every word FILL."""
    import torch
    from attentive_dfprior_amd import _lib
    query = {'f32': 'packed_floats', 'ht': 'packed_ht_words'}.get(fmt, 'packed_h_words')
    out = torch.full((sizes(_lib.lib(), name)[query],), FILL, dtype=torch.int32, device=device)
    return out.view(torch.float32) if fmt == 'f32' else out


def entry_image(name, fmt, flat, status, two_part_entry=False):
    """One image through the library's single-image C entries, into a buffer pre-filled with FILL.  'h' / 'g' / 'hg':
    adfp_pack_split_image (two_part_entry: 'hg' through adfp_pack_decoder_h / adfp_pack_attention_h instead); 'ht':
    adfp_pack_decoder_ht / adfp_pack_attention_ht; 'f32': adfp_pack_decoder / adfp_pack_attention."""
    from attentive_dfprior_amd import _lib
    L, out = _lib.lib(), filled(name, fmt, flat.device)
    tail = (_lib.ptr(flat), _lib.ptr(out)) + (() if fmt == 'f32' else (C.c_void_p(status.data_ptr()),)) + (_lib.current_stream(flat.device),)
    if fmt in ('h', 'g', 'hg') and not two_part_entry:
        which = {'h': _lib.IMAGE_H, 'g': _lib.IMAGE_G, 'hg': _lib.IMAGE_H | _lib.IMAGE_G}[fmt]
        rc = L.adfp_pack_split_image(_lib.NET_ID[name], which, *tail)
    else:
        entry = {'hg': 'h', 'ht': 'ht', 'f32': ''}[fmt]
        if name == 'att':
            rc = getattr(L, 'adfp_pack_attention' + ('_' + entry if entry else ''))(*tail)
        else:
            rc = getattr(L, 'adfp_pack_decoder' + ('_' + entry if entry else ''))(_lib.DEC_KIND[name], *tail)
    _lib.check(rc, f'{name} {fmt}')
    return out


def loaded(sd):
    import attentive_dfprior_amd as A
    dec = A.DF()
    dec.load_state_dict(sd)
    return dec.to('cuda:0')


def record(path=FIXTURE):
    import torch
    from attentive_dfprior_amd import _lib
    out = {'sizes': {n: sizes(_lib.lib(), n) for n in NETS}, 'cases': {}}
    for case, sd in state_dicts().items():
        dec, status = loaded(sd), _lib.new_status_word()
        rec = out['cases'][case] = {'flat': {}, 'hg': {}, 'ht': {}, 'f32': {}}
        for n in NETS:
            flat = dec.flat_weights(n)
            rec['flat'][n] = sha(flat)
            for fmt in ('hg', 'ht', 'f32'):
                rec[fmt][n] = sha(entry_image(n, fmt, flat, status))
        torch.cuda.synchronize()
        rec['status'] = int(status[0])
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    record(*sys.argv[1:2])
