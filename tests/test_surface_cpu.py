"""The drop-in boundary is the reference's Python function surface: every function of its hot-path modules must exist
under the same name in the product's module of the same name.  The reference's function names are stored in
tests/golden/reference_surface.json (written by tests/golden/make_fixtures.py from the reference tree)."""
import importlib
import json
import os

import pytest

SURFACE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_surface.json')
MODULES = {
    'distributions/gaussian.py': 'vmp_for_svae_amd.distributions.gaussian',
    'distributions/niw.py': 'vmp_for_svae_amd.distributions.niw',
    'distributions/dirichlet.py': 'vmp_for_svae_amd.distributions.dirichlet',
    'distributions/student_t.py': 'vmp_for_svae_amd.distributions.student_t',
    'models/gmm.py': 'vmp_for_svae_amd.models.gmm',
    'models/smm.py': 'vmp_for_svae_amd.models.smm',
    'models/svae.py': 'vmp_for_svae_amd.models.svae',
    'data.py': 'vmp_for_svae_amd.data',
    'helpers/tf_utils.py': 'vmp_for_svae_amd.helpers.tf_utils',
    'helpers/scheduling.py': 'vmp_for_svae_amd.helpers.scheduling',
}
# plotting / TensorBoard / script entry points of the model files are outside the hot path
OUT_OF_SCOPE = {'main', 'plot', 'visualise', 'visualize'}


@pytest.mark.parametrize('rel,mod', sorted(MODULES.items()))
def test_every_reference_function_has_a_counterpart(rel, mod):
    import vmp_for_svae_amd  # noqa: F401
    names = json.load(open(SURFACE))[rel]
    assert names                                       # every module of the surface has functions in the reference
    m = importlib.import_module(mod)
    missing = [n for n in names if not hasattr(m, n) and not any(n.startswith(p) for p in OUT_OF_SCOPE)]
    assert not missing, (rel, missing)


def test_niw_outer_is_the_batched_outer_product():
    import torch
    from vmp_for_svae_amd.distributions import niw
    a, b = torch.arange(6.).reshape(2, 3), torch.arange(6., 12.).reshape(2, 3)
    assert torch.equal(niw._outer(a, b), torch.einsum('kd,ke->kde', a, b))


def test_read_from_tfrec_file_round_trip(tmp_path):
    """reference data.py:179-213: a TFRecord file written here byte by byte (record framing + tf.train.Example wire format, the
    label once as a plain and once as a packed int64 list) comes back as (pixels / 255, labels); binarise=True gives +-1."""
    import struct
    import numpy as np
    from vmp_for_svae_amd import data

    def varint(v):
        out = b''
        while True:
            c = v & 0x7F
            v >>= 7
            out += bytes([c | (0x80 if v else 0)])
            if not v:
                return out

    def ld(fn, payload):
        return varint((fn << 3) | 2) + varint(len(payload)) + payload

    def example(img, label, packed):
        f_img = ld(1, ld(1, img.tobytes()))                                             # Feature.bytes_list.value
        ints = ld(1, varint(label)) if packed else (varint((1 << 3) | 0) + varint(label))  # Int64List.value packed / plain
        f_lab = ld(3, ints)
        feats = ld(1, ld(1, b'image_raw') + ld(2, f_img)) + ld(1, ld(1, b'label') + ld(2, f_lab))
        return ld(1, feats)

    rng = np.random.Generator(np.random.PCG64(0))
    D = 28
    imgs = rng.integers(0, 256, size=(5, D), dtype=np.uint8)
    labels = [3, 0, 9, 300, 7]
    path = tmp_path / 'toy.tfrecords'
    with open(path, 'wb') as f:
        for i in range(5):
            ex = example(imgs[i], labels[i], packed=bool(i & 1))
            f.write(struct.pack('<Q', len(ex)) + b'\0\0\0\0' + ex + b'\0\0\0\0')
    X, lab = data.read_from_tfrec_file(str(path), D)
    assert np.array_equal(lab, labels) and np.allclose(X, imgs.astype(np.float32) / 255)
    Xb, _ = data.read_from_tfrec_file([str(path)], D, binarise=True, seed=1)
    assert set(np.unique(Xb)) <= {-1.0, 1.0} and (Xb[imgs == 255] == 1).all() and (Xb[imgs == 0] == -1).all()


def test_make_minibatch_reads_the_image_data_sets_when_present(tmp_path):
    """reference data.py:13-33: <datadir>/mnist_new/{train,test}.tfrecords with 784 pixels -> one-hot labels of 10 classes; absent files
    are a FileNotFoundError (the repository ships none)."""
    import struct
    import numpy as np
    from vmp_for_svae_amd import data
    with pytest.raises(FileNotFoundError):
        data.make_minibatch('mnist', path_datadir=str(tmp_path), size_minibatch=-1, device='cpu')

    def varint(v):
        out = b''
        while True:
            c = v & 0x7F
            v >>= 7
            out += bytes([c | (0x80 if v else 0)])
            if not v:
                return out

    def ld(fn, payload):
        return varint((fn << 3) | 2) + varint(len(payload)) + payload
    rng = np.random.Generator(np.random.PCG64(2))
    d = tmp_path / 'mnist_new'
    d.mkdir()
    want = {}
    for split, n in (('train', 6), ('test', 3)):
        imgs = rng.integers(0, 256, size=(n, 784), dtype=np.uint8)
        labs = rng.integers(0, 10, size=n)
        want[split] = (imgs, labs)
        with open(d / (split + '.tfrecords'), 'wb') as f:
            for i in range(n):
                feats = ld(1, ld(1, b'image_raw') + ld(2, ld(1, ld(1, imgs[i].tobytes())))) + \
                        ld(1, ld(1, b'label') + ld(2, ld(3, ld(1, varint(int(labs[i]))))))
                ex = ld(1, feats)
                f.write(struct.pack('<Q', len(ex)) + b'\0\0\0\0' + ex + b'\0\0\0\0')
    y_tr, l_tr, y_te, l_te = data.make_minibatch('mnist', path_datadir=str(tmp_path), size_minibatch=-1, device='cpu')
    assert tuple(y_tr.shape) == (6, 784) and tuple(l_te.shape) == (3, 10)
    assert np.allclose(y_tr.numpy(), want['train'][0].astype(np.float32) / 255)
    assert np.array_equal(l_tr.numpy().argmax(1), want['train'][1]) and np.array_equal(l_te.numpy().argmax(1), want['test'][1])
