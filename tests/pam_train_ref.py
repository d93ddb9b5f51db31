"""float64 references and fp32 error bounds for ganet's position-attention part nodes under train() (csrc/pam.hip:
agrl_pam_pool_train, agrl_pam_pool_backward, agrl_pam_combine_train, agrl_pam_combine_backward, agrl_col_sum), for
``bounds.check_rounded(..., out_dtype=torch.float32)``. Written like train_ref.graph_matrix_backward_ref: ``exact`` is the float64
value of the formulas in include/agrl_hip.h on the fp32 operands the kernel reads, and where an output sits behind the energy,
the softmax and several products, the bound is the rounding of every fp32 step propagated to first order through them and handed
to check_rounded as ``slack``; where a kernel consumes a vector it also returns (abar), the consumer is referenced on the kernel's
own values with a plain chain length, so a last-bit difference upstream does not loosen the bar downstream.

Constants, u = 2^-24 (bounds.U32), all read off csrc/pam.hip:
  energy      E[p,q] = sum_c Q[p,c] K[q,c], one fmaf chain over the Cq channels:           Cq u sum |Q||K|
  softmax     d = E - max (one subtraction: u |d|), expf: 1 ulp = 2 u relative (the ROCm device-library / HIP math API table lists
              expf at 1 ulp), row sum e0 + e1 and six shuffle steps of positive terms: 7 u, the quotient: u. With A = softmax(E)
              and dA_q = A_q (dE_q - sum_q' A_q' dE_q'):
                  eA[p,q] = A[p,q] (eE[p,q] + sum_q' A[p,q'] eE[p,q'] + u (|d[p,q]| + 2) + sum_q' A[p,q'] u (|d[p,q']| + 2) + 8 u)
  abar        sequential sum over the L rows, then the quotient:  eabar[q] = sum_p eA[p,q] / L + (L + 1) u abar[q]
  xbar        fmaf chain over the L positions on the kernel's abar: n_acc = L;  xmean: L additions and the quotient: n_acc = L + 1
  dabar       a lane's ceil(C / 64) fmafs and six shuffle steps:   edab[q] = (ceil(C / 64) + 6) u sum_c |X[q,c]| |dxbar[c]|
  g = A dabar one product, one fmaf, six shuffle steps (8 u):       eg[p] = sum_q (eA |dab| + A edab) + 8 u sum_q A |dab|
  dE          t = dab[q] - g[p] (u |t|), A t (u), 1 / L rounded (u), the product (u):
                  edE = (eA |t| + A (edab[q] + eg[p] + u |t|)) / L + 3 u |dE|
  dQ, dK      fmaf chains over L:   edQ[p,c] = sum_q edE[p,q] |K[q,c]| + L u sum_q |dE||K|   (dK alike with Q and dE^T);
              the levels add into dqk one after the other: nlev u sum_levels |dQ_level| more
  dX          per level fmaf(dxmean, 1 / L, acc) and fmaf(abar, dxbar, .) on the kernel's abar: 1 / L rounded, two fmafs: 3 per level
  combine     y + bv and one fmaf: 2.  dy = gamma dn: 1.  dxmean = 2 dn: exact.
  column sums a thread's rows of its chunk in order, then the chunks in order (hip_ops.col_sum_plan): rpc + chunks; dbv one
              product more; dgamma: (y + bv) 1, the fmaf chain rpc, chunks, a thread's ceil(C / 256) channels, 6 shuffle steps, 2
A plain module (like train_ref.py): the tests import it. Everything here runs on the CPU."""
import torch

from bounds import U32

MAXL = 128


def slices(splits, h):
    """[(r0, r1)] per part, in part order: h // n rows each, the remainder dropped."""
    return [((h // n) * j, (h // n) * (j + 1)) for n in splits for j in range(n)]


def levels(splits, h):
    """[(rows per slice, slices, first part)] per pyramid level."""
    out, off = [], 0
    for n in splits:
        out.append((h // n, n, off))
        off += n
    return out


def covered_rows(splits, h):
    """bool (h): rows at least one slice covers."""
    m = torch.zeros(h, dtype=torch.bool)
    for r0, r1 in slices(splits, h):
        m[r0:r1] = True
    return m


def attention_ref(Q, K):
    """Q, K (F,L,Cq) fp32 -> A, eA (F,L,L), abar, eabar (F,L) in float64 (docstring above)."""
    u = U32
    Q, K = Q.double(), K.double()
    L, Cq = Q.shape[1], Q.shape[2]
    E = Q @ K.transpose(1, 2)
    eE = Cq * u * (Q.abs() @ K.abs().transpose(1, 2))
    d = E - E.max(dim=2, keepdim=True).values
    A = torch.softmax(E, dim=2)
    r = u * (d.abs() + 2)
    eA = A * (eE + (A * eE).sum(2, keepdim=True) + r + (A * r).sum(2, keepdim=True) + 8 * u)
    abar = A.mean(dim=1)
    eabar = eA.sum(dim=1) / L + (L + 1) * u * abar
    return A, eA, abar, eabar


def forward_ref(x, qk, splits, abar_got):
    """agrl_pam_pool_train. x (F,h,w,C), qk (F,h,w,2Cq) fp32, abar_got (F,P,128) the kernel's own abar ->
    dict: abar (exact, slack) (F,P,128), xbar (exact, mag, n_acc) on abar_got, xmean (exact, mag, n_acc); n_acc (1,P,1) tensors;
    row_max: list per part of the float64 attention's row maxima (F,L)."""
    F_, h, w, C = x.shape
    Cq = qk.shape[-1] // 2
    P = sum(splits)
    ab, eab = torch.zeros((F_, P, MAXL), dtype=torch.float64), torch.zeros((F_, P, MAXL), dtype=torch.float64)
    xb, xbm = torch.zeros((F_, P, C), dtype=torch.float64), torch.zeros((F_, P, C), dtype=torch.float64)
    xm, xmm = torch.zeros_like(xb), torch.zeros_like(xb)
    nL = torch.zeros((1, P, 1), dtype=torch.float64)
    row_max = []
    for part, (r0, r1) in enumerate(slices(splits, h)):
        L = (r1 - r0) * w
        X = x[:, r0:r1].reshape(F_, L, C).double()
        A, _, abar, eabar = attention_ref(qk[:, r0:r1, :, :Cq].reshape(F_, L, Cq), qk[:, r0:r1, :, Cq:].reshape(F_, L, Cq))
        row_max.append(A.max(dim=2).values)
        ab[:, part, :L], eab[:, part, :L] = abar, eabar
        a_own = abar_got[:, part, :L].double()
        xb[:, part] = torch.einsum('fq,fqc->fc', a_own, X)
        xbm[:, part] = torch.einsum('fq,fqc->fc', a_own.abs(), X.abs())
        xm[:, part], xmm[:, part] = X.mean(1), X.abs().mean(1)
        nL[0, part, 0] = L
    return {"abar": (ab, eab), "xbar": (xb, xbm, nL), "xmean": (xm, xmm, nL + 1), "row_max": row_max}


def backward_ref(x, qk, dxbar, dxmean, splits, abar_got):
    """agrl_pam_pool_backward -> dict: dx (exact, mag, n_acc) on the kernel's own abar, dqk (exact, slack), abar (exact, slack)."""
    u = U32
    F_, h, w, C = x.shape
    Cq = qk.shape[-1] // 2
    P = sum(splits)
    nlev = len(splits)
    dx, dxm = torch.zeros((F_, h, w, C), dtype=torch.float64), torch.zeros((F_, h, w, C), dtype=torch.float64)
    dqk, edqk, mqk = (torch.zeros((F_, h, w, 2 * Cq), dtype=torch.float64) for _ in range(3))
    ab, eab = torch.zeros((F_, P, MAXL), dtype=torch.float64), torch.zeros((F_, P, MAXL), dtype=torch.float64)
    lane_chain = -(-C // 64) + 6
    for part, (r0, r1) in enumerate(slices(splits, h)):
        L = (r1 - r0) * w
        X = x[:, r0:r1].reshape(F_, L, C).double()
        Q, K = qk[:, r0:r1, :, :Cq].reshape(F_, L, Cq), qk[:, r0:r1, :, Cq:].reshape(F_, L, Cq)
        A, eA, abar, eabar = attention_ref(Q, K)
        Q, K = Q.double(), K.double()
        ab[:, part, :L], eab[:, part, :L] = abar, eabar
        db, dm = dxbar[:, part].double(), dxmean[:, part].double()
        a_own = abar_got[:, part, :L].double()
        dx[:, r0:r1] += (a_own.unsqueeze(2) * db.unsqueeze(1) + dm.unsqueeze(1) / L).reshape(F_, r1 - r0, w, C)
        dxm[:, r0:r1] += (a_own.abs().unsqueeze(2) * db.abs().unsqueeze(1) + dm.abs().unsqueeze(1) / L).reshape(F_, r1 - r0, w, C)
        dab = torch.einsum('fqc,fc->fq', X, db)
        edab = lane_chain * u * torch.einsum('fqc,fc->fq', X.abs(), db.abs())
        g = torch.einsum('fpq,fq->fp', A, dab)
        eg = (eA * dab.abs().unsqueeze(1) + A * edab.unsqueeze(1)).sum(2) + 8 * u * torch.einsum('fpq,fq->fp', A, dab.abs())
        t = dab.unsqueeze(1) - g.unsqueeze(2)
        dE = A * t / L
        edE = (eA * t.abs() + A * (edab.unsqueeze(1) + eg.unsqueeze(2) + u * t.abs())) / L + 3 * u * dE.abs()
        dQ, dK = dE @ K, dE.transpose(1, 2) @ Q
        mQ, mK = dE.abs() @ K.abs(), dE.abs().transpose(1, 2) @ Q.abs()
        eQ = edE @ K.abs() + L * u * mQ
        eK = edE.transpose(1, 2) @ Q.abs() + L * u * mK
        shape = (F_, r1 - r0, w, Cq)
        dqk[:, r0:r1, :, :Cq] += dQ.reshape(shape)
        dqk[:, r0:r1, :, Cq:] += dK.reshape(shape)
        edqk[:, r0:r1, :, :Cq] += eQ.reshape(shape)
        edqk[:, r0:r1, :, Cq:] += eK.reshape(shape)
        mqk[:, r0:r1, :, :Cq] += dQ.abs().reshape(shape)
        mqk[:, r0:r1, :, Cq:] += dK.abs().reshape(shape)
    return {"dx": (dx, dxm, 3 * nlev), "dqk": (dqk, edqk + nlev * u * mqk), "abar": (ab, eab)}


def combine_ref(y, bv, xmean, gamma):
    """nodes = gamma (y + bv) + 2 xmean -> exact, mag, n_acc."""
    g = float(gamma)
    y, bv, xm = y.double(), bv.double(), xmean.double()
    return g * (y + bv) + 2 * xm, abs(g) * (y.abs() + bv.abs()) + 2 * xm.abs(), 2


def combine_backward_ref(dn, y, bv, gamma, plan):
    """agrl_pam_combine_backward; plan = hip_ops.col_sum_plan(rows) -> dict name -> (exact, mag, n_acc)."""
    chunks, rpc = plan
    g = float(gamma)
    C = dn.shape[-1]
    d2, y2, b = dn.double().reshape(-1, C), y.double().reshape(-1, C), bv.double()
    prod, pmag = d2 * (y2 + b), d2.abs() * (y2.abs() + b.abs())
    return {"dy": (g * dn.double(), abs(g) * dn.double().abs(), 1),
            "dxmean": (2 * dn.double(), 2 * dn.double().abs(), 0),
            "dbv": (g * d2.sum(0), abs(g) * d2.abs().sum(0), rpc + chunks + 1),
            "dgamma": (prod.sum().view(1), pmag.sum().view(1), 1 + rpc + chunks + -(-C // 256) + 8)}


def col_sum_ref(x2d, plan):
    chunks, rpc = plan
    return x2d.double().sum(0), x2d.double().abs().sum(0), rpc + chunks


def attn_pool_forward_ref(nodes):
    """agrl_row_sqnorm + agrl_attn_pool_bnneck's attention branch (csrc/pool.hip): n_sp = |f_sp|, a_sp = n_sp / max(sum_s n_sp,
    1e-12), att_f = (1 / P) sum_p sum_s a_sp f_sp -> exact, mag, n_acc. With t = ceil(C / 64) + 6 (a lane's fmafs of the squared
    norm and the six shuffle steps): n carries (t / 2 + 1) u (the square root halves the relative error), the sum over the frames
    S more, the quotient one: a carries at most (t + S + 3) u; the fmaf chain over the frames S, the sum over the parts P, the
    division by P one: t + 2 S + P + 4 against mag = (1 / P) sum_p sum_s a_sp |f_sp|."""
    B, S, P, C = nodes.shape
    f = nodes.double()
    n = f.pow(2).sum(3, keepdim=True).sqrt()
    a = n / n.sum(1, keepdim=True).clamp(min=1e-12)
    t = -(-C // 64) + 6
    return (a * f).sum(1).mean(1), (a * f.abs()).sum(1).mean(1), t + 2 * S + P + 4
