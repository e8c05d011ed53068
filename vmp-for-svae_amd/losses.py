"""Evaluation metrics - mirror of the hot-path-adjacent part of reference losses.py:
weighted_mse (:9-38), diagonal_gaussian_logprob (:83-145), purity (:313-349), and the missing-data imputation
measurements imputation_mse (:148-170), imputation_losses (:173-246), generate_missing_data_mask (:249-285),
perturb_data (:288-310).  The (N,K,S,D)-sized reductions run
in csrc/vmp_loglike.hip (vmp_eval_cell_metrics); the cluster/label contingency table of `purity` re-uses the
mixture moment kernel (sum_n r_nk * labels_nc is exactly its first-moment block).

Streaming evaluation (streaming_metrics, streaming_imputation_losses): the same measurements on an evaluation set of any size.  The
set is walked in chunks of plan_eval_chunks rows; per chunk the encoder, the E-step with in-kernel noise at the chunk's row offset and
the decoder forward with the metric epilogue (vmp_decoder_eval_fwd) run, so that no (N,K,S,.)-sized tensor of the whole set - and no
(.,K,S,Dy) tensor at all - exists.  The results do not depend on the chunking."""
import math

import numpy as np
import torch

from . import _lib as L
from ._lib import VmpError
from .models import _mix, _svae_ops, svae, vae


def _cell_metrics(y, mean, var, logw, mask, want_mse, want_lse, mask_mse=False):
    y = L.dev_f32(y, 'y_true')
    mean = L.dev_f32(mean, 'y_pred / mean')
    N, K, S, D = mean.shape
    if tuple(y.shape) != (N, D):
        raise AssertionError('y_true must have shape (N,D)')
    var = None if var is None else L.dev_f32(var, 'var', (N, K, S, D))
    per_s = 0
    if logw is not None:
        if tuple(logw.shape) == (N, K, S):
            per_s = 1
        elif tuple(logw.shape) != (N, K):
            raise AssertionError('log_weights must have shape (N,K) or (N,K,S)')
        logw = L.dev_f32(logw, 'log_weights')
    m8 = None
    if mask is not None:
        if tuple(mask.shape) != (N, D):
            raise AssertionError('mask must have shape (N,D)')
        m8 = mask.to(torch.uint8).contiguous()
    f32 = dict(dtype=torch.float32, device=y.device)
    mse = torch.empty(N, K, **f32) if want_mse else None
    lse = torch.empty(N, K, **f32) if want_lse else None
    L.check(L.lib().vmp_eval_cell_metrics(L.ptr(y), L.ptr(mean), L.ptr(var), L.ptr(logw), per_s, L.ptr(m8), 1 if mask_mse else 0, N, K, S, D,
                                          L.ptr(mse), L.ptr(lse), L.stream()), 'vmp_eval_cell_metrics')
    return mse, lse


def weighted_mse(y_true, y_pred, r_nk_pred, name='mse'):
    """reference losses.py:9-38: mean_n sum_k r_nk mean_s sum_d (y_nd - yhat_nksd)^2."""
    mse, _ = _cell_metrics(y_true, y_pred, None, None, None, True, False)
    if tuple(r_nk_pred.shape) != tuple(mse.shape):
        raise AssertionError('r_nk_pred must have shape (N,K)')
    return (mse * r_nk_pred).sum(1).mean()


def diagonal_gaussian_logprob(y_true, mean, var, log_weights, mask=None, name='gauss_logprob'):
    """reference losses.py:83-145: mean_n log sum_k exp(log_weights) 1/S sum_s N(y_n | mean_nks, diag var_nks)."""
    _, lse = _cell_metrics(y_true, mean, var, log_weights, mask, False, True)
    return torch.logsumexp(lse, dim=1).mean()


def bernoulli_logprob(y_true_bin, logits, log_weights=None, missing_data_mask=None, name='bernoulli_logprob'):
    """reference losses.py:41-80.  logits (N,S,D) or, with log_weights (N,K) / (N,K,S), (N,K,S,D); y in {-1,+1}.
    Kept as written: the sample average subtracts S, not log S (losses.py:76-78)."""
    if log_weights is None:
        N, S, D = logits.shape
        lg4 = logits.unsqueeze(1)
    else:
        N, K, S, D = logits.shape
        if tuple(log_weights.shape) not in ((N, K), (N, K, S)):
            raise AssertionError('log_weights must have shape (N,K) or (N,K,S)')
        if log_weights.dim() == 2:
            log_weights = log_weights.unsqueeze(2)
        lg4 = logits
    if tuple(y_true_bin.shape) != (N, D):
        raise AssertionError('y_true_bin must have shape (N,D)')
    rows = _svae_ops.BernoulliRowsFn.apply(y_true_bin, lg4.contiguous(), missing_data_mask)      # (N,K|1,S)
    if log_weights is not None:
        logprobs = torch.logsumexp(rows + log_weights, dim=1)                                   # (N,S)
    else:
        logprobs = rows[:, 0, :]
    return (torch.logsumexp(logprobs, dim=-1) - float(S)).mean()


def purity(r_nk, labels, eps=1e-10, name='purity'):
    """reference losses.py:313-349.  labels: one-hot (N,C).  Returns (entropy, purity)."""
    N, K = r_nk.shape
    N_k, N_kc = _contingency(r_nk, labels)
    return _purity_from_table(N_k, N_kc, N, eps)


def _contingency(r_nk, labels):
    """(N_k (K), N_kc (K,C)) = (sum_n r_nk, sum_n r_nk labels_nc), fp64, through the mixture moment kernel"""
    C = labels.shape[1]
    r = L.dev_f32(r_nk, 'r_nk')
    cols = []
    for c0 in range(0, C, L.MAX_D):                                    # the moment kernel takes up to 8 columns
        lab = L.dev_f32(labels[:, c0:c0 + L.MAX_D].float().contiguous(), 'labels')
        st = _mix.raw_stats(lab, r, pivot=torch.zeros(lab.shape[1], dtype=torch.float32, device=r.device))
        cols.append(st[:, 2:2 + lab.shape[1]])
        N_k = st[:, 0]
    return N_k, torch.cat(cols, dim=1)


def _purity_from_table(N_k, N_kc, N, eps=1e-10):
    p_kc = N_kc / (N_k + eps).unsqueeze(1)
    cluster_entropy = -(p_kc * torch.log(p_kc + eps)).sum(1)
    entropy = (N_k / N * cluster_entropy).sum()
    pur = (N_k / N * p_kc.max(dim=1).values).sum()
    return entropy.float(), pur.float()


def imputation_mse(y_true, y_pred, r_nk_pred, missing_data_mask, name='imp_mse'):
    """reference losses.py:148-170: 1/N sum_nk r_nk mean_s sum_d mask_nd (y_nd - yhat_nksd)^2 (observed entries are
    zeroed in both the truth and the prediction, i.e. they do not count)."""
    mse, _ = _cell_metrics(y_true, y_pred, None, None, missing_data_mask, True, False, mask_mse=True)
    if tuple(r_nk_pred.shape) != tuple(mse.shape):
        raise AssertionError('r_nk_pred must have shape (N,K)')
    return (mse * r_nk_pred).sum() / y_true.shape[0]


def generate_missing_data_mask(y, noise_ratio=0.3, mask_type='random', seed=0, name='make_mask'):
    """reference losses.py:249-285: a random but constant boolean (N,D) mask (same numpy RandomState draw), or the
    image-shaped 'quarter' / 'lower_half' / 'left_half' masks."""
    N, D = y.shape
    mask = np.zeros(N * D, dtype=bool)
    if mask_type == 'random':
        nb = int(N * D * noise_ratio)
        missing = np.random.RandomState(seed).choice(np.arange(N * D), size=nb, replace=False)
        mask[missing] = True
    else:
        side = np.sqrt(D)
        assert side.is_integer()
        side = int(side)
        half = side // 2
        mask = mask.reshape(N, side, side)
        if mask_type == 'quarter':
            mask[:, half:side, :half] = True
        elif mask_type == 'lower_half':
            mask[:, half:side, :side] = True
        elif mask_type == 'left_half':
            mask[:, :side, :half] = True
        else:
            raise NotImplementedError("The mask type '%s' does not exist." % mask_type)
    return torch.as_tensor(mask.reshape(N, D), device=y.device)


def perturb_data(y, missing_data_mask, seed, decoder_type='standard', name='perturb_data', noise=None):
    """reference losses.py:288-310: masked entries are replaced by N(0,1) noise (`noise` (N,D) injects the draw that
    tf.random_normal makes in the reference)."""
    m = missing_data_mask.to(y.dtype)
    if noise is None:
        g = torch.Generator(device=y.device).manual_seed(int(seed))
        if decoder_type == 'standard':
            noise = torch.randn(y.shape, generator=g, device=y.device, dtype=y.dtype)
        elif decoder_type == 'bernoulli':                 # fair coin in {-1,+1} (losses.py:301-306)
            noise = (torch.rand(y.shape, generator=g, device=y.device) < 0.5).to(y.dtype) * 2.0 - 1.0
        else:
            raise NotImplementedError
    return (1.0 - m) * y + m * noise


def imputation_losses(y_true, missing_data_mask, imputation_method, nb_samples_pert=100, nb_samples_rec=100, seed=0,
                      decoder_type='standard', name='imputation_losses', noise=None):
    """reference losses.py:173-246.  imputation_method(y_perturbed) -> (mean (N,K,S,D), var (N,K,S,D), log_r_nk (N,K)).
    Returns (expected masked MSE over the perturbations, log-likelihood of the missing entries under the mixture of all
    nb_samples_pert * S imputations).  The reference concatenates every imputation along S before one
    diagonal_gaussian_logprob; the same number is accumulated here perturbation by perturbation:
    log 1/(P S) sum_{p,s} e^{..} = logsumexp_p(lse_p) - log P with lse_p the per-cell value of one perturbation.
    `noise` (P,N,D) injects the perturbation draws; by default perturbation p uses seed + p (the reference passes the
    SAME op seed to every tf.random_normal, losses.py:207)."""
    if decoder_type not in ('standard', 'bernoulli'):
        raise NotImplementedError
    bern = decoder_type == 'bernoulli'
    # for the MSE the binary data in {-1,1} is compared as {0,1} (losses.py:193-198)
    y_cmp = torch.where(y_true == -1, torch.zeros_like(y_true), torch.ones_like(y_true)) if bern else y_true
    mse = 0.0
    lse_acc = None
    rows_all, lw_all = [], []
    for p in range(nb_samples_pert):
        y_pert = perturb_data(y_true, missing_data_mask, seed + p, decoder_type=decoder_type,
                              noise=None if noise is None else noise[p])
        with torch.no_grad():
            mean, out2, log_r_nk = imputation_method(y_pert)
        if bern:
            m_p, _ = _cell_metrics(y_cmp, mean, None, None, missing_data_mask, True, False, mask_mse=True)
            rows_all.append(_svae_ops.BernoulliRowsFn.apply(y_true, out2.contiguous(), missing_data_mask))
            lw_all.append(log_r_nk.unsqueeze(2).expand(-1, -1, out2.shape[2]))
        else:
            m_p, lse_p = _cell_metrics(y_true, mean, out2, log_r_nk, missing_data_mask, True, True, mask_mse=True)
            lse_acc = lse_p if lse_acc is None else torch.logaddexp(lse_acc, lse_p)
        mse = mse + (m_p * torch.exp(log_r_nk)).sum() / y_true.shape[0]
    expected_mse = mse / nb_samples_pert
    if bern:
        # bernoulli_logprob on the imputations concatenated along S (losses.py:231-241): only (N,K,S)-sized tensors
        rows, lw = torch.cat(rows_all, dim=2), torch.cat(lw_all, dim=2)
        logprobs = torch.logsumexp(rows + lw, dim=1)
        loglike = (torch.logsumexp(logprobs, dim=-1) - float(rows.shape[2])).mean()
    else:
        loglike = torch.logsumexp(lse_acc - math.log(nb_samples_pert), dim=1).mean()
    return expected_mse, loglike


# ---------------------------------------------------------------------------------------------------------
# Streaming evaluation
# ---------------------------------------------------------------------------------------------------------
DEFAULT_EVAL_WORKSPACE = 256 << 20      # a memory bound (measured: larger chunks are slightly faster, cache residency of x does not show)


def _mlp_row_words(hidden, out_dim):
    """fp32 words per input row that the torch MLP (vae.make_nnet) holds at its peak: every hidden activation (they stay referenced
    until the head is done), one more of the widest layer (the pre-activation beside its tanh), and six head-sized tensors
    ([raw1 | raw2] (2), softplus, the shortcut x W + b1, and the two outputs)."""
    hidden = [int(u) for u in hidden]
    return sum(hidden) + (max(hidden) if hidden else 0) + 6 * out_dim


def _eval_row_bytes(K, S, Ld, Dy, in_kernel, fused, hidden=(), enc_hidden=None):
    """Bytes of chunk-sized buffers per evaluated row - every tensor the chunk loop of _stream_cells allocates:
    x (K,S,L); the (K,L,S) noise workspace for shapes outside the in-kernel generator; the per-sample-row pair (K,S,2) of
    vmp_decoder_eval_fwd - or, for a 'standard' decoder outside the fused range (fused=False, hidden = its hidden widths), what the
    torch MLP holds per sample row (_mlp_row_words: hidden activations and head tensors, mean and var among them); the encoder's two
    outputs (L) - or the torch encoder's tensors when enc_hidden is given; and the (K)-sized cell values log z, T', mse, lse plus two
    temporaries of the contractions."""
    dec = 2 * K * S if fused else K * S * _mlp_row_words(hidden, Dy)
    enc = 2 * Ld if enc_hidden is None else _mlp_row_words(enc_hidden, Ld)
    words = K * S * Ld + (0 if in_kernel else K * Ld * S) + dec + enc + 6 * K
    return 4 * words


def _rng_in_kernel(K, Ld, S):
    return L.lib().vmp_svae_rng_in_kernel(K, Ld, S)


def plan_eval_chunks(N, K, S, L, Dy, max_workspace_bytes=DEFAULT_EVAL_WORKSPACE, in_kernel=None, fused=True, hidden=(), enc_hidden=None):
    """Rows per chunk of the streaming evaluation: the largest number whose chunk-sized buffers (_eval_row_bytes) fit
    max_workspace_bytes, at most N.  in_kernel: whether the E-step draws its noise in the kernel (default: the library's answer,
    vmp_svae_rng_in_kernel - a host query).  fused=False / hidden, enc_hidden: a decoder / an encoder outside the fused kernels' range
    runs the torch MLP per chunk, whose hidden activations (widths `hidden`) are counted.  Raises VmpError when the budget does not
    hold one row."""
    N, K, S, L_, Dy = int(N), int(K), int(S), int(L), int(Dy)
    if min(N, K, S, L_, Dy) < 1:
        raise VmpError('plan_eval_chunks: N, K, S, L, Dy must be positive')
    if in_kernel is None:
        in_kernel = bool(_rng_in_kernel(K, L_, S))
    per_row = _eval_row_bytes(K, S, L_, Dy, in_kernel, fused, hidden, enc_hidden)
    rows = int(max_workspace_bytes) // per_row
    if rows < 1:
        raise VmpError('plan_eval_chunks: a budget of %d bytes does not hold one evaluation row (K=%d S=%d L=%d Dy=%d need %d bytes)'
                       % (int(max_workspace_bytes), K, S, L_, Dy, per_row))
    rows = min(rows, N)
    while rows * K * S >= 2 ** 31:                                      # the decoder kernels index sample rows with 32 bits
        rows = (rows + 1) // 2
    return rows


def _check_head(decoder_layers):
    head = decoder_layers[-1][1]
    if head == 'bernoulli':
        raise NotImplementedError("streaming evaluation covers Gaussian ('standard') decoder heads; a 'bernoulli' head is outside "
                                  "its limit - use imputation_losses / bernoulli_logprob on the materialised outputs")
    if head != 'standard':
        raise NotImplementedError("streaming evaluation: decoder head '%s' is not supported" % (head,))


def _stream_cells(y_in, y_cmp, phi_gmm, encoder_layers, decoder_layers, nb_samples, mask, mask_mse, stddev_init_nn, seed,
                  max_workspace_bytes, on_chunk=None):
    """The chunk loop.  y_in (N,Dy) goes through the encoder; the decoder's outputs are compared with y_cmp (N,Dy).
    Returns (mse (N,K), lse (N,K) with log_weights = log z, log_z (N,K)) - the per-cell values of _cell_metrics on the whole set.
    on_chunk(c0, c1, log_z_chunk): called per chunk (purity's contingency table)."""
    _check_head(decoder_layers)
    y_in = L.dev_f32(y_in, 'y')
    N, Dy = y_in.shape
    y_cmp = L.dev_f32(y_cmp, 'y_true', (N, Dy))
    dev = y_in.device
    S = int(nb_samples)
    prep = svae.recognition_prep(phi_gmm, None)                         # K-sized: once, outside the chunk loop
    K, Ld = prep[0].shape
    fused = vae.fused_decoder_eligible(Ld, decoder_layers)
    dec_params = vae.decoder_variables(Ld, decoder_layers, stddev_init_nn, seed, dev) if fused else None
    in_kernel = bool(L.lib().vmp_svae_rng_in_kernel(K, Ld, S))
    enc_fused = vae._fused_mlp_eligible(Dy, encoder_layers)
    rows = plan_eval_chunks(N, K, S, Ld, Dy, max_workspace_bytes, in_kernel=in_kernel, fused=fused,
                            hidden=[u for u, _ in decoder_layers[:-1]], enc_hidden=None if enc_fused else [u for u, _ in encoder_layers[:-1]])
    m8 = None if mask is None else mask.to(torch.uint8).contiguous()
    if m8 is not None and tuple(m8.shape) != (N, Dy):
        raise AssertionError('mask must have shape (N,D)')
    f32 = dict(dtype=torch.float32, device=dev)
    mse, lse, log_z = torch.empty(N, K, **f32), torch.empty(N, K, **f32), torch.empty(N, K, **f32)
    ws = torch.empty(rows * K * S * 8, dtype=torch.uint8, device=dev) if fused else None
    for c0 in range(0, N, rows):
        c1 = min(N, c0 + rows)
        phi_enc = vae.make_encoder(y_in[c0:c1], layerspecs=encoder_layers, stddev_init=stddev_init_nn, seed=seed)
        x, lz, _, _ = svae.e_step(phi_enc, phi_gmm, S, noise=_svae_ops.PhiloxNoise(seed, S, row0=c0, at=True), prep=prep)
        mk = None if m8 is None else m8[c0:c1]
        if fused:
            m_c, l_c = _svae_ops.decoder_eval(x, y_cmp[c0:c1], dec_params, logw=lz, mask=mk, mask_mse=mask_mse, ws=ws)
        else:                                                           # 'standard' head outside the fused range: materialised per chunk
            mean, var = vae.make_decoder(x, layerspecs=decoder_layers, stddev_init=stddev_init_nn, seed=seed)
            m_c, l_c = _cell_metrics(y_cmp[c0:c1], mean, var, lz, mk, True, True, mask_mse=mask_mse)
            del mean, var
        mse[c0:c1], lse[c0:c1], log_z[c0:c1] = m_c, l_c, lz
        if on_chunk is not None:
            on_chunk(c0, c1, lz)
        del x, lz, phi_enc, m_c, l_c                                    # before the next chunk allocates: one chunk resident at a time
    return mse, lse, log_z


def streaming_metrics(y, phi_gmm, encoder_layers, decoder_layers, nb_samples, *, labels=None, missing_data_mask=None, mask_mse=False,
                      stddev_init_nn=0.01, seed=0, max_workspace_bytes=DEFAULT_EVAL_WORKSPACE):
    """The test-time measurement of the reference driver (experiments.py:270-304: svae.inference with nb_samples_te samples, then
    weighted_mse, diagonal_gaussian_logprob and purity) on a set of any size, in bounded memory.  Returns a dict:
    mse_n (N,) = sum_k r_nk mse_nk, loli_n (N,) = logsumexp_k lse_nk, log_z (N,K), the scalars mse, loli (means over n of the two
    vectors, summed in one fixed order: independent of the chunking) and - with one-hot labels (N,C) - entropy, purity.
    missing_data_mask (N,Dy): the log-likelihood counts masked entries only (losses.py:118-124), and so does the squared error under
    mask_mse.  The E-step noise is the in-kernel Philox stream keyed by `seed` (row n draws the stream of row n whatever the chunk)."""
    with torch.no_grad():
        N = y.shape[0]
        table = []

        def on_chunk(c0, c1, lz):
            N_k, N_kc = _contingency(torch.exp(lz), labels[c0:c1])
            if not table:
                table.extend([N_k.double().clone(), N_kc.double().clone()])
            else:
                table[0] += N_k
                table[1] += N_kc
        mse_nk, lse_nk, log_z = _stream_cells(y, y, phi_gmm, encoder_layers, decoder_layers, nb_samples, missing_data_mask, mask_mse,
                                              stddev_init_nn, seed, max_workspace_bytes, on_chunk if labels is not None else None)
        mse_n = (mse_nk * torch.exp(log_z)).sum(1)
        loli_n = torch.logsumexp(lse_nk, dim=1)
        out = {'mse_n': mse_n, 'loli_n': loli_n, 'log_z': log_z, 'mse': float(mse_n.mean()), 'loli': float(loli_n.mean())}
        if labels is not None:
            e, p = _purity_from_table(table[0], table[1], N)
            out['entropy'], out['purity'] = float(e), float(p)
    return out


def streaming_imputation_losses(y, missing_data_mask, phi_gmm, encoder_layers, decoder_layers, nb_samples_pert=100, nb_samples_rec=100,
                                *, stddev_init_nn=0.01, seed=0, max_workspace_bytes=DEFAULT_EVAL_WORKSPACE, noise=None):
    """imputation_losses ('standard' decoder) with svae.inference as the imputation method, streamed: per perturbation p the WHOLE
    (N,D) array is perturbed as perturb_data does (seed + p, or noise[p]), the perturbed set is walked in chunks, and the
    log-add-exp over p stays on (N,K).  The E-step draws the same key for every p (the reference passes one seed, experiments.py:365-372).
    Returns (expected masked MSE, log-likelihood of the missing entries)."""
    with torch.no_grad():
        N = y.shape[0]
        mse = 0.0
        lse_acc = None
        for p in range(nb_samples_pert):
            y_pert = perturb_data(y, missing_data_mask, seed + p, noise=None if noise is None else noise[p])
            m_p, lse_p, log_r = _stream_cells(y_pert.contiguous(), y, phi_gmm, encoder_layers, decoder_layers, nb_samples_rec,
                                              missing_data_mask, True, stddev_init_nn, seed, max_workspace_bytes)
            lse_acc = lse_p if lse_acc is None else torch.logaddexp(lse_acc, lse_p)
            mse = mse + (m_p * torch.exp(log_r)).sum() / N
        return mse / nb_samples_pert, torch.logsumexp(lse_acc - math.log(nb_samples_pert), dim=1).mean()
