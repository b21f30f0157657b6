"""Host-side application helpers on top of the evaluator: the reference's `app/LinearHelperCKKS.cuh`
MatmulHelper and the CKKS polynomial (coefficient) encoding it uses, `CKKSEncoderCuda::encodePolynomial / decodePolynomial`
(`src/ckks_cuda.cu:455-575, 983-1055`).  Pure packing logic: every ciphertext operation goes through `troy_amd.api`.

The helper's batch dimension (independent input rows) IS the evaluator's batch dimension here: `Cipher2d[i]` is ONE batched
ciphertext holding block i of every input row, so a matmul over B rows costs the same launches as over one.
`encodePolynomial` exists only in the reference's CUDA encoder (no CPU twin to pin against): it is restated from the CUDA
source and checked by round trip and by the plaintext matmul (floating point, tolerance in the tests).
"""
import math

import numpy as np

from . import api, capi


def _c_round(x):
    """C round(): half away from zero (numpy rounds half to even)."""
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


class CKKSPolyEncoder:
    def __init__(self, context):
        if context.scheme != capi.CKKS:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "unsupported scheme")
        self.context = context
        self.slots = context.N // 2

    def encodePolynomial(self, values, limbs, scale):
        """values: up to N doubles (coefficients) -> uint64 [limbs][N], NTT form, plaintext scale = `scale`."""
        ctx, N = self.context, self.context.N
        v = np.zeros(N, dtype=np.float64)
        values = np.asarray(values, dtype=np.float64)
        if values.size > N:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "values_size is too large")
        v[: values.size] = values
        c = _c_round(v * scale)
        primes = ctx.coeff_modulus[:limbs]
        max_coeff = float(np.max(np.abs(v * scale))) if N else 0.0
        bits = int(math.ceil(math.log2(max(max_coeff, 1.0)))) + 1
        if bits >= sum(int(p).bit_length() for p in primes):
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "encoded values are too large")
        out = np.zeros((limbs, N), dtype=np.uint64)
        neg = c < 0
        if bits <= 64:
            mag = np.abs(c).astype(np.uint64)
            for l, p in enumerate(primes):
                r = mag % np.uint64(p)
                out[l] = np.where(neg & (r != 0), np.uint64(p) - r, r)
        else:  # the exact integer value of the (rounded) double, reduced per prime
            ints = [int(x) for x in np.abs(c)]
            for l, p in enumerate(primes):
                r = np.array([x % int(p) for x in ints], dtype=np.uint64)
                out[l] = np.where(neg & (r != 0), np.uint64(p) - r, r)
        buf = api.DeviceBuffer.from_numpy(out)
        ctx.ntt(buf, limbs, primes)
        return buf.to_numpy().reshape(limbs, N)

    def decodePolynomial(self, plain_ntt, scale):
        """uint64 [limbs][N] (NTT form) -> N doubles: inverse NTT, CRT composition, centred, times 1/scale."""
        ctx, N = self.context, self.context.N
        plain_ntt = np.ascontiguousarray(plain_ntt, dtype=np.uint64)
        limbs = plain_ntt.shape[0]
        primes = [int(p) for p in ctx.coeff_modulus[:limbs]]
        buf = api.DeviceBuffer.from_numpy(plain_ntt)
        ctx.ntt(buf, limbs, primes, inverse=True)
        x = buf.to_numpy().reshape(limbs, N)
        q = 1
        for p in primes:
            q *= p
        # CRT: sum_l x_l * (q/p_l) * ((q/p_l)^-1 mod p_l) mod q
        acc = [0] * N
        for l, p in enumerate(primes):
            m = q // p
            w = m * pow(m % p, -1, p)
            xl = x[l]
            for j in range(N):
                acc[j] += int(xl[j]) * w
        half = (q + 1) >> 1
        inv = 1.0 / scale
        out = np.empty(N, dtype=np.float64)
        for j in range(N):
            a = acc[j] % q
            out[j] = float(a - q if a >= half else a) * inv
        return out


def _encrypt(encryptor, plain):
    """the reference's helpers encrypt with the SECRET key (encryptSymmetric, LinearHelperCKKS.cuh:213-222); an Encryptor that only holds a
    public key falls back to it"""
    return encryptor.encryptSymmetric(plain) if getattr(encryptor, "sk", None) is not None else encryptor.encrypt(plain)


def _ceil_div(a, b):
    return (a + b - 1) // b


def _serialize_terms(evaluator, outputs, required_of, stream):
    """stream order of the reference (batch outer, output block / channel inner); each batched ciphertext is brought to
    coefficient form ONCE"""
    hosts = [ct.coeff_host(evaluator) for ct in outputs]
    for b in range(outputs[0].batch):
        for cid, ct in enumerate(outputs):
            ct.saveTerms(stream, evaluator, required_of(cid), index=b, coeff_host=hosts[cid])


def _deserialize_terms(evaluator, context, batch, count, required_of, stream):
    parts = [[None] * batch for _ in range(count)]
    meta = [None] * count
    for b in range(batch):
        for cid in range(count):
            data, ntt, scale, cf = api.Ciphertext.load_terms_host(context, stream, required_of(cid))
            parts[cid][b], meta[cid] = data[0], (ntt, scale, cf)
    outs = []
    for cid in range(count):
        ntt, scale, cf = meta[cid]
        ct = api.Ciphertext.from_numpy(context, np.stack(parts[cid]), False, scale, cf)
        if ntt:
            evaluator.transformToNttInplace(ct)
        outs.append(ct)
    return outs


class MatmulHelper:
    """app/LinearHelperCKKS.cuh:104-360, same packing: an input block of `blockHeight` entries is a polynomial x_0 + x_1 X + ..,
    a weight block (h x w) puts W[i][j] at degree j*h + h-1-i, so that coefficient (j+1)*h - 1 of the product is sum_i x_i W[i][j]."""

    def __init__(self, batchSize, inputDims, outputDims, slotCount):
        self.batchSize, self.inputDims, self.outputDims, self.slotCount = batchSize, inputDims, outputDims, slotCount
        self._determine_block()
        self.encodedWeights = None

    def _determine_block(self):  # LinearHelperCKKS.cuh:112-123
        height, width, slots = self.inputDims, self.outputDims, self.slotCount * 2
        self.blockHeight = self.blockWidth = 0
        bt = height + width + 1
        for i in range(1, height + 1):
            w = min(slots // i, width)
            if w == 0:
                break
            t = _ceil_div(height, i) + _ceil_div(width, w)
            if t < bt:
                self.blockHeight, self.blockWidth, bt = i, w, t

    def encodeWeights(self, encoder, limbs, weights, scale):
        """weights: [inputDims][outputDims] doubles -> Plain2d (list of rows of DeviceBuffer [limbs][N], NTT form)"""
        W = np.asarray(weights, dtype=np.float64).reshape(self.inputDims, self.outputDims)
        h, w, slots = self.blockHeight, self.blockWidth, self.slotCount * 2
        rows = []
        for li in range(0, self.inputDims, h):
            ui = min(li + h, self.inputDims)
            row = []
            for lj in range(0, self.outputDims, w):
                uj = min(lj + w, self.outputDims)
                vec = np.zeros(slots)
                for j in range(lj, uj):
                    for i in range(li, ui):
                        vec[(j - lj) * h + h - (i - li) - 1] = W[i, j]
                row.append(api.DeviceBuffer.from_numpy(encoder.encodePolynomial(vec, limbs, scale)))
            rows.append(row)
        self.encodedWeights, self.weightScale = rows, scale
        return rows

    def encryptInputs(self, encryptor, encoder, limbs, inputs, scale):
        """inputs: [batchSize][inputDims] doubles -> Cipher2d: list over input blocks of ONE batched ciphertext each"""
        X = np.asarray(inputs, dtype=np.float64).reshape(self.batchSize, self.inputDims)
        ctx = encoder.context
        out = []
        for lj in range(0, self.inputDims, self.blockHeight):
            uj = min(lj + self.blockHeight, self.inputDims)
            cts = np.stack([_encrypt(encryptor, encoder.encodePolynomial(X[b, lj:uj], limbs, scale)) for b in range(self.batchSize)])
            out.append(api.Ciphertext.from_numpy(ctx, cts, True, scale, 1))
        return out

    def matmul(self, evaluator, a):
        """Cipher2d x encoded weights -> list over output blocks of one batched ciphertext (same order of additions as the
        reference: block row i = 0 initialises, the others are added in order)"""
        if len(a) != len(self.encodedWeights):
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "Input size incorrect.")
        rows, cols = len(self.encodedWeights), len(self.encodedWeights[0])
        if rows <= 16:  # one pass per output block: sum_i a[i] (x) W[i][j], every operand read once (same residues as the loop below)
            return [evaluator.multiplyPlainAccumulate([a[i] for i in range(rows)], [self.encodedWeights[i][j] for i in range(rows)], self.weightScale) for j in range(cols)]
        outs = [None] * cols
        for i, wrow in enumerate(self.encodedWeights):
            for j, wp in enumerate(wrow):
                prod = a[i].copy()
                evaluator.multiplyPlainInplace(prod, wp, self.weightScale)
                if i == 0:
                    outs[j] = prod
                else:
                    evaluator.addInplace(outs[j], prod)
        return outs

    def decryptOutputs(self, evaluator, encoder, secret_key_dev, outputs):
        """-> [batchSize][outputDims] doubles (device decryption, host decode)"""
        dec = np.zeros((self.batchSize, self.outputDims))
        interval, vecsize = self.blockHeight, self.blockWidth
        for cid, li in enumerate(range(0, self.outputDims, vecsize)):
            ui = min(li + vecsize, self.outputDims)
            pts = evaluator.decrypt(outputs[cid], secret_key_dev)  # [batch][limbs][N]
            for b in range(self.batchSize):
                buf = encoder.decodePolynomial(pts[b], outputs[cid].scale)
                for j in range(li, ui):
                    dec[b, j] = buf[(j - li + 1) * interval - 1]
        return dec

    def _required(self, cid):  # LinearHelperCKKS.cuh:326-337: coefficient (j+1)*blockHeight - 1 of output block cid
        li = cid * self.blockWidth
        ui = min(li + self.blockWidth, self.outputDims)
        return [(j - li + 1) * self.blockHeight - 1 for j in range(li, ui)]

    def serializeOutputs(self, evaluator, outputs, stream):
        """LinearHelperCKKS.cuh:326-339: only the coefficients decryptOutputs reads travel (saveTerms)"""
        _serialize_terms(evaluator, outputs, self._required, stream)

    def deserializeOutputs(self, evaluator, context, stream):  # LinearHelperCKKS.cuh:341-358
        return _deserialize_terms(evaluator, context, self.batchSize, _ceil_div(self.outputDims, self.blockWidth), self._required, stream)


class Conv2dHelper:
    """app/LinearHelperCKKS.cuh:362-716: valid (no padding, stride 1) 2-D convolution by polynomial multiplication.  An image block
    (h x w) of channel k sits at degrees k*h*w + i*w + j; the flipped kernel of input channel j at slot (channelSlots-1-j);
    the output pixel (i, j) of the block is read at degree (channelSlots-1)*h*w + (h-yh+i)*w + (w-yw+j).  Images larger than
    sqrt(N) per side are cut into overlapping blocks, which multiplies the batch (`getTotalBatchSize`)."""

    def __init__(self, batchSize, imageHeight, imageWidth, kernelHeight, kernelWidth, inputChannels, outputChannels, slotCount):
        self.batchSize, self.imageHeight, self.imageWidth = batchSize, imageHeight, imageWidth
        self.kernelHeight, self.kernelWidth = kernelHeight, kernelWidth
        self.inputChannels, self.outputChannels, self.slotCount = inputChannels, outputChannels, slotCount
        max_size = int(math.isqrt(slotCount * 2))
        if imageHeight > max_size or imageWidth > max_size:
            self.blockHeight = self.blockWidth = max_size
            self.blocked = True
        else:
            self.blockHeight, self.blockWidth, self.blocked = imageHeight, imageWidth, False
        self.encodedWeights = None

    def _grid(self):
        kh, kw = self.kernelHeight - 1, self.kernelWidth - 1
        return _ceil_div(self.imageHeight - kh, self.blockHeight - kh), _ceil_div(self.imageWidth - kw, self.blockWidth - kw)

    def getTotalBatchSize(self):
        if not self.blocked:
            return self.batchSize
        sh, sw = self._grid()
        return self.batchSize * sh * sw

    def encodeWeights(self, encoder, limbs, weights, scale):
        """weights [outputChannels][inputChannels][kh][kw] -> Plain2d [oc][input-channel group] of DeviceBuffer"""
        W = np.asarray(weights, dtype=np.float64).reshape(self.outputChannels, self.inputChannels, self.kernelHeight, self.kernelWidth)
        bs = self.blockHeight * self.blockWidth
        cs = (self.slotCount * 2) // bs
        rows = []
        for oc in range(self.outputChannels):
            row = []
            for lic in range(0, self.inputChannels, cs):
                uic = min(lic + cs, self.inputChannels)
                spread = np.zeros((cs, self.blockHeight, self.blockWidth))
                for j in range(lic, uic):
                    spread[cs - 1 - (j - lic), : self.kernelHeight, : self.kernelWidth] = W[oc, j, ::-1, ::-1]
                row.append(api.DeviceBuffer.from_numpy(encoder.encodePolynomial(spread.reshape(-1), limbs, scale)))
            rows.append(row)
        self.encodedWeights, self.weightScale = rows, scale
        return rows

    def _split(self, X):
        if not self.blocked:
            return X
        kh, kw = self.kernelHeight - 1, self.kernelWidth - 1
        sh, sw = self._grid()
        out = np.zeros((self.batchSize * sh * sw, self.inputChannels, self.blockHeight, self.blockWidth))
        for b in range(self.batchSize):
            for i in range(sh):
                for j in range(sw):
                    si, sj = i * (self.blockHeight - kh), j * (self.blockWidth - kw)
                    ui, uj = min(si + self.blockHeight, self.imageHeight), min(sj + self.blockWidth, self.imageWidth)
                    out[b * sh * sw + i * sw + j, :, : ui - si, : uj - sj] = X[b, :, si:ui, sj:uj]
        return out

    def encryptInputs(self, encryptor, encoder, limbs, inputs, scale):
        """inputs [batchSize][inputChannels][H][W] -> list over input-channel groups of ONE batched ciphertext (batch = total batch)"""
        X = self._split(np.asarray(inputs, dtype=np.float64).reshape(self.batchSize, self.inputChannels, self.imageHeight, self.imageWidth))
        total, interval = X.shape[0], self.blockHeight * self.blockWidth
        cs = (self.slotCount * 2) // interval
        ctx = encoder.context
        out = []
        for c0 in range(0, self.inputChannels, cs):
            c1 = min(c0 + cs, self.inputChannels)
            cts = np.stack([_encrypt(encryptor, encoder.encodePolynomial(X[b, c0:c1].reshape(-1), limbs, scale)) for b in range(total)])
            out.append(api.Ciphertext.from_numpy(ctx, cts, True, scale, 1))
        return out

    def conv2d(self, evaluator, a):
        """-> list over output channels of one batched ciphertext (sum over input-channel groups in order)"""
        if len(a) <= 16:  # one pass per output channel (troyhip_multiply_plain_accumulate), as in MatmulHelper.matmul
            return [evaluator.multiplyPlainAccumulate(list(a), [self.encodedWeights[oc][i] for i in range(len(a))], self.weightScale) for oc in range(self.outputChannels)]
        outs = []
        for oc in range(self.outputChannels):
            acc = None
            for i, ai in enumerate(a):
                prod = ai.copy()
                evaluator.multiplyPlainInplace(prod, self.encodedWeights[oc][i], self.weightScale)
                if acc is None:
                    acc = prod
                else:
                    evaluator.addInplace(acc, prod)
            outs.append(acc)
        return outs

    def decryptOutputs(self, evaluator, encoder, secret_key_dev, outputs):
        """-> [batchSize][outputChannels][H-kh+1][W-kw+1] doubles"""
        interval = self.blockHeight * self.blockWidth
        cs = (self.slotCount * 2) // interval
        yh, yw = self.blockHeight - self.kernelHeight + 1, self.blockWidth - self.kernelWidth + 1
        oyh, oyw = self.imageHeight - self.kernelHeight + 1, self.imageWidth - self.kernelWidth + 1
        sh, sw = self._grid() if self.blocked else (1, 1)
        ret = np.zeros((self.batchSize, self.outputChannels, oyh, oyw))
        for c in range(self.outputChannels):
            pts = evaluator.decrypt(outputs[c], secret_key_dev)
            for b in range(pts.shape[0]):
                buf = encoder.decodePolynomial(pts[b], outputs[c].scale)
                blk = buf[(cs - 1) * interval: cs * interval].reshape(self.blockHeight, self.blockWidth)[self.blockHeight - yh:, self.blockWidth - yw:]
                ob, si, sj = b // (sh * sw), (b % (sh * sw)) // sw, b % sw
                i1, j1 = min(si * yh + yh, oyh), min(sj * yw + yw, oyw)
                if si * yh < oyh and sj * yw < oyw:
                    ret[ob, c, si * yh: i1, sj * yw: j1] = blk[: i1 - si * yh, : j1 - sj * yw]
        return ret

    def _required(self, cid):  # LinearHelperCKKS.cuh:684-690: the last channel slot of every output polynomial
        interval = self.blockHeight * self.blockWidth
        st = ((self.slotCount * 2) // interval - 1) * interval
        return list(range(st, st + interval))

    def serializeOutputs(self, evaluator, outputs, stream):  # LinearHelperCKKS.cuh:684-696
        _serialize_terms(evaluator, outputs, self._required, stream)

    def deserializeOutputs(self, evaluator, context, stream):  # LinearHelperCKKS.cuh:698-713
        return _deserialize_terms(evaluator, context, self.getTotalBatchSize(), self.outputChannels, self._required, stream)


class DiagonalMatvec:
    """y = M x for a plain d x d matrix M and an encrypted vector x by the diagonal method (Halevi-Shoup), as ONE hoisted call
    (Evaluator.rotate*PlainSumHoisted): y = sum_r diag_r (.) rot(x, r), the nonzero diagonals only.  d is a power of two
    dividing the row length N / 2; x is tiled with period d over the row (BFV / BGV: over both rows), and so is y.  One key per nonzero diagonal: from a few
    dozen diagonals on, DiagonalMatvecBSGS below (baby-step / giant-step) needs far fewer keys."""

    def __init__(self, context, matrix):
        m = np.asarray(matrix)
        row = context.N // 2
        if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 1 or m.shape[0] & (m.shape[0] - 1) or row % m.shape[0]:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "matrix must be d x d, d a power of two dividing the row length N / 2")
        self.context, self.matrix, self.d, self.row = context, m, m.shape[0], row
        k = np.arange(self.d)
        diags = [m[k, (k + r) % self.d] for r in range(self.d)]  # diag_r[k] = M[k][(k + r) mod d]
        self.steps = [r for r in range(self.d) if np.any(diags[r] != 0)]
        self.diagonals = {r: np.tile(diags[r], row // self.d) for r in self.steps}
        self.plains, self.plain_scale = None, 1.0

    def requiredSteps(self):
        """the rotation steps whose Galois keys apply() needs (step 0 needs none)"""
        return [r for r in self.steps if r]

    def encodeDiagonals(self, encoder, scale=None):
        """the key-level NTT plaintexts of the nonzero diagonals: encoder = BatchEncoder (BFV / BGV) or CKKSEncoder with `scale`"""
        ctx = self.context
        K = ctx.key_limbs
        if ctx.scheme == capi.CKKS:
            if scale is None:
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "CKKS diagonals need a scale")
            self.plains = [api.DeviceBuffer.from_numpy(encoder.encode(self.diagonals[r], scale, limbs=K)) for r in self.steps]
            self.plain_scale = float(scale)
        else:
            ev = api.Evaluator(ctx)
            self.plains = [ev.transformPlainToNtt(api.DeviceBuffer.from_numpy(encoder.encode(np.concatenate([self.diagonals[r]] * 2))), K) for r in self.steps]
            self.plain_scale = 1.0
        return self.plains

    def apply(self, evaluator, ct, galois_keys):
        """the single hoisted call; ct encrypts x tiled with period d"""
        if self.plains is None:
            raise capi.LogicError(capi.LOGIC_ERROR, "encodeDiagonals has not been called")
        if not self.steps:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "the matrix is zero")
        # a key set with grouped digits goes to the members that take one
        name = ("rotateVector" if self.context.scheme == capi.CKKS else "rotateRows") + "PlainSumHoisted" + ("Grouped" if galois_keys.special_primes is not None else "")
        fn = getattr(evaluator, name)
        return fn(ct, self.steps, self.plains, galois_keys, self.plain_scale)


class DiagonalMatvecBSGS:
    """y = M x as DiagonalMatvec, by baby steps and giant steps (Evaluator.rotate*PlainSumBsgs): with r = i n1 + j,
        y = sum_i rot( sum_j rot(diag_{i n1 + j}, -i n1) (.) rot(x, j), i n1 ),        rot(v, s)[k] = v[k + s],
    so n1 = baby_steps baby rotations and d / n1 giant rotations serve all d diagonals: n1 + d / n1 - 2 Galois keys instead of d - 1, and one key stream
    per baby and per giant instead of one per diagonal.  Zero diagonals are absent terms; a baby step or a giant row that only zero diagonals use needs no
    key.  baby_steps: a power of two dividing d (default: the one nearest sqrt(6 d)), with baby_steps and d / baby_steps <= 64."""

    def __init__(self, context, matrix, baby_steps=None):
        m = np.asarray(matrix)
        row = context.N // 2
        if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 1 or m.shape[0] & (m.shape[0] - 1) or row % m.shape[0]:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "matrix must be d x d, d a power of two dividing the row length N / 2")
        d = m.shape[0]
        if baby_steps is None:
            baby_steps = min((1 << e for e in range(d.bit_length()) if (1 << e) <= 64 and d >> e <= 64), key=lambda n1: abs(n1 - (6 * d) ** 0.5), default=0)
        n1 = int(baby_steps)
        if n1 < 1 or n1 & (n1 - 1) or d % n1 or n1 > 64 or d // n1 > 64:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "baby_steps must be a power of two dividing d, with baby_steps and d / baby_steps at most 64")
        self.context, self.matrix, self.d, self.row, self.n1, self.n2 = context, m, d, row, n1, d // n1
        k = np.arange(d)
        diags = [m[k, (k + r) % d] for r in range(d)]  # diag_r[k] = M[k][(k + r) mod d]
        self.steps = [r for r in range(d) if np.any(diags[r] != 0)]
        # pt[i][j] encodes rot(diag_{i n1 + j}, -i n1): the tiled diagonal rotates as a tile
        self.diagonals = {r: np.tile(np.roll(diags[r], (r // n1) * n1), row // d) for r in self.steps}
        self.baby_steps = list(range(n1))
        self.giant_steps = [i * n1 for i in range(self.n2)]
        self.plains, self.plain_scale = None, 1.0

    def requiredSteps(self):
        """the rotation steps whose Galois keys apply() needs: the baby steps and the giant steps a nonzero diagonal uses (step 0 needs none)"""
        return sorted({r % self.n1 for r in self.steps if r % self.n1} | {(r // self.n1) * self.n1 for r in self.steps if r // self.n1})

    def encodeDiagonals(self, encoder, scale=None):
        """the n2 x n1 table of key-level NTT plaintexts (None: a zero diagonal): encoder = BatchEncoder (BFV / BGV) or CKKSEncoder with `scale`"""
        ctx = self.context
        K = ctx.key_limbs
        if ctx.scheme == capi.CKKS:
            if scale is None:
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "CKKS diagonals need a scale")
            enc = lambda v: api.DeviceBuffer.from_numpy(encoder.encode(v, scale, limbs=K))
            self.plain_scale = float(scale)
        else:
            ev = api.Evaluator(ctx)
            enc = lambda v: ev.transformPlainToNtt(api.DeviceBuffer.from_numpy(encoder.encode(np.concatenate([v] * 2))), K)
            self.plain_scale = 1.0
        self.plains = [[enc(self.diagonals[i * self.n1 + j]) if i * self.n1 + j in self.diagonals else None for j in range(self.n1)] for i in range(self.n2)]
        return self.plains

    def apply(self, evaluator, ct, galois_keys):
        """the single baby-step / giant-step call; ct encrypts x tiled with period d"""
        if self.plains is None:
            raise capi.LogicError(capi.LOGIC_ERROR, "encodeDiagonals has not been called")
        if not self.steps:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "the matrix is zero")
        # a key set with grouped digits goes to the members that take one
        name = ("rotateVector" if self.context.scheme == capi.CKKS else "rotateRows") + "PlainSumBsgs" + ("Grouped" if galois_keys.special_primes is not None else "")
        fn = getattr(evaluator, name)
        return fn(ct, self.baby_steps, self.giant_steps, self.plains, galois_keys, self.plain_scale)


# ---------------------------------------------------------------- private information retrieval
# A composition of public calls: the client sends ONE ciphertext and d RGSW ciphertexts, the server expands the first (Evaluator.expandCoefficients),
# scans the database with it (Evaluator.multiplyPlainMatrix) and folds the columns with the RGSWs (Evaluator.cmux).  The database holds D0 * 2^d
# records, each a plaintext polynomial of N coefficients mod t; record i = r + D0 * j lies at row r, column j.  BFV and BGV, per-prime keys.  The
# client makes the RGSWs of the column bits itself: converting RLWE encryptions of the bits on the server is not part of this.
def _pir_shape(context, D0, d):
    D0, d = int(D0), int(d)
    if context.scheme not in (capi.BFV, capi.BGV):
        raise capi.LogicError(capi.LOGIC_ERROR, "unsupported scheme")
    if D0 < 1 or D0 & (D0 - 1) or D0 > context.N or not 0 <= d <= 20:
        raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "PIR: D0 is a power of two, at most N, and the database has D0 * 2^d records, d <= 20")
    return D0, d


def _window(ct, first, count):
    """items first .. first + count - 1 of a dense batch, as a batch of their own (no copy)"""
    item = ct.bstride
    out = api.Ciphertext(ct.context, count, ct.size(), ct.limbs, ct.is_ntt_form, ct.scale, ct.correction_factor, ct.capacity,
                         buf=api._BufferWindow(ct.buf, first * item, count * item))
    return out


class PIRClient:
    def __init__(self, context, keygen, encryptor, decryptor, D0, d):
        self.D0, self.d = _pir_shape(context, D0, d)
        self.context, self.keygen, self.encryptor, self.decryptor = context, keygen, encryptor, decryptor

    def galoisKeys(self):
        """the keys the server's expansion needs: the elements KeyGenerator.expansionElts(D0), generated on the device"""
        elts = self.keygen.expansionElts(self.D0)
        return self.keygen.createGaloisKeys(elts, device=True) if elts else api.GaloisKeys(self.context)

    def query(self, i):
        """record i = r + D0 * j -> (one Ciphertext encrypting the monomial x^r, d RGSWCiphertexts of the bits of j, the highest bit first)"""
        i = int(i)
        if not 0 <= i < self.D0 << self.d:
            raise capi.OutOfRange(capi.OUT_OF_RANGE, "PIR: no such record")
        r, j = i % self.D0, i // self.D0
        mono = np.zeros(r + 1, dtype=np.uint64)
        mono[r] = 1
        ct = api.Ciphertext.from_numpy(self.context, self.encryptor.encrypt(mono)[None])
        bits = [np.array([(j >> (self.d - 1 - k)) & 1], dtype=np.uint64) for k in range(self.d)]
        return ct, self.keygen.createRGSWBatch(bits)

    def recover(self, answer):
        """the record an answer (one ciphertext, coefficient form) encrypts: N coefficients mod t"""
        return self.decryptor.decrypt(answer.cpu()[0], correction_factor=answer.correction_factor)

    def noiseBudget(self, answer):
        return self.decryptor.invariantNoiseBudget(answer.cpu()[0])


class PIRServer:
    def __init__(self, context, records, D0):
        """records: uint64 [D0 * 2^d][N] (or fewer coefficients per record), coefficients mod t.  They are lifted and transformed ONCE, at the first data
        level, into [D0][2^d][limbs][N] on the device"""
        records = np.ascontiguousarray(records, dtype=np.uint64)
        if records.ndim != 2 or records.shape[0] < 1 or records.shape[0] % int(D0) or not 1 <= records.shape[1] <= context.N:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "PIR: records is [D0 * 2^d][up to N coefficients]")
        cols = records.shape[0] // int(D0)
        if cols & (cols - 1):
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "PIR: D0 is a power of two, at most N, and the database has D0 * 2^d records, d <= 20")
        self.D0, self.d = _pir_shape(context, D0, cols.bit_length() - 1)
        self.context, self.cols, self.limbs = context, cols, context.first_limbs
        self.evaluator = ev = api.Evaluator(context)
        n = records.shape[1]
        by_row = np.ascontiguousarray(records.reshape(cols, self.D0, n).transpose(1, 0, 2))  # record r + D0 * j -> [r][j]
        self.plains = ev.transformPlainToNtt(api.DeviceBuffer.from_numpy(by_row), self.limbs, n_coeffs=n, count=self.D0 * cols)
        api.synchronize()

    def _scan(self, query, galois_keys):
        """steps 1 - 4 on a batch of B queries -> ONE Ciphertext of cols * B items in coefficient form, column after column"""
        ev = self.evaluator
        if query.size() != 2 or query.is_ntt_form or query.limbs != self.limbs:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "PIR: a query is a fresh size-2 ciphertext in coefficient form at the first data level")
        rows = ev.expandCoefficients(query, self.D0, galois_keys)
        whole = api.Ciphertext(self.context, self.D0 * query.batch, 2, self.limbs, buf=rows[0].buf.owner)  # the rows are windows of one buffer, row after row
        whole._absorb(rows[0].struct())
        ev.transformToNttInplace(whole)
        out = ev.multiplyPlainMatrix(whole, self.plains, self.D0, self.cols)
        columns = api.Ciphertext(self.context, self.cols * query.batch, 2, self.limbs, buf=out[0].buf.owner)
        columns._absorb(out[0].struct())
        ev.transformFromNttInplace(columns)
        return columns

    def scan(self, query, galois_keys):
        """the scan stage alone: `cols` ciphertexts, column j encrypting record r + D0 * j of the query's row r"""
        columns = self._scan(query, galois_keys)
        return [_window(columns, j * query.batch, query.batch) for j in range(self.cols)]

    def _fold(self, columns, selectors):
        """d rounds of cmux over the halves of the contiguous column buffer: the selector of the highest bit first"""
        if len(selectors) != self.d:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "PIR: one selector per bit of the column index")
        for sel in selectors:
            half = columns.batch // 2
            columns = self.evaluator.cmux(sel, _window(columns, 0, half), _window(columns, half, half))
        return columns

    def answer(self, query, selectors, galois_keys):
        """one query -> one ciphertext encrypting the record"""
        if query.batch != 1:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "PIR: answer takes one query; answerBatch takes several")
        return self._fold(self._scan(query, galois_keys), selectors)

    def answerBatch(self, queries, selectors, galois_keys):
        """B clients: the expansion and the scan run once over the batch of their queries -- the database is streamed once for all of them -- and the
        folds per client, because an RGSW multiplies every item of a batch"""
        B = len(queries)
        if B < 1 or len(selectors) != B or any(q.batch != 1 or q.bstride != queries[0].bstride for q in queries):
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "PIR: one single query and one list of selectors per client")
        q0 = queries[0]
        item = q0.bstride
        batch = api.Ciphertext(self.context, B, q0.size(), q0.limbs, q0.is_ntt_form, q0.scale, q0.correction_factor, q0.capacity)
        for b, q in enumerate(queries):
            batch.buf.copy_from(q.buf, item, 0, b * item)
        columns = self._scan(batch, galois_keys)  # [cols][B]
        out = []
        for b in range(B):
            mine = api.Ciphertext(self.context, self.cols, 2, self.limbs, columns.is_ntt_form, columns.scale, columns.correction_factor)
            for j in range(self.cols):
                mine.buf.copy_from(columns.buf, columns.bstride, (j * B + b) * columns.bstride, j * columns.bstride)
            out.append(self._fold(mine, selectors[b]))
        return out


# ---- look-up tables on LWE samples: a composition of public calls, extract -> modulus switch -> blind rotation -> extract.
class LookupTable:
    """A function on Z_(2N) as a negacyclic test vector.  `f` maps a message m in [0, 2^t_bits) to a value mod t; the phases [0, N) are cut into 2^t_bits
    equal windows, table[phi] = f(phi 2^t_bits // N), and the other half is forced: table[phi + N] = -table[phi].  The polynomial v with v_0 = table[0]
    and v_(N - phi) = -table[phi] has table[phi] as the constant coefficient of v x^phi, which is what Evaluator.blindRotate leaves encrypted."""

    def __init__(self, context, f, t_bits):
        if context.scheme not in (capi.BFV, capi.BGV):
            raise capi.LogicError(capi.LOGIC_ERROR, "unsupported scheme")
        N, t = context.N, context.plain_modulus
        t_bits = int(t_bits)
        if not 0 <= t_bits <= N.bit_length() - 1:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "LookupTable: 2^t_bits windows, at most N")
        self.context, self.t_bits = context, t_bits
        self.table = np.array([int(f((phi << t_bits) // N)) % t for phi in range(N)], dtype=np.uint64)
        self.poly = np.zeros(N, dtype=np.uint64)
        self.poly[0] = self.table[0]
        self.poly[1:] = (t - self.table[:0:-1].astype(object)) % t

    def value(self, phi):
        """the constant coefficient of poly x^phi in R_t, phi in Z_(2N)"""
        N, t = self.context.N, self.context.plain_modulus
        phi = int(phi) % (2 * N)
        return int(self.table[phi]) if phi < N else (t - int(self.table[phi - N])) % t

    def test_vector(self, limbs):
        """[limbs][N] canonical residues: round(q poly / t) for BFV (q the product of the level's primes), the plain lift for BGV"""
        ctx, t = self.context, self.context.plain_modulus
        primes = ctx.coeff_modulus[:int(limbs)]
        q = 1
        for p in primes:
            q *= p
        vals = [(q * int(v) + t // 2) // t if ctx.scheme == capi.BFV else int(v) for v in self.poly]
        return np.array([[v % p for v in vals] for p in primes], dtype=np.uint64)

    def apply(self, evaluator, ct_batch, terms, key, limbs=None, scratch_limit_words=0, lwe_key=None):
        """the table on the coefficients `terms` of every item of a BFV / BGV batch -> (rotated, lwes): modSwitchTo one limb, extractLWEs, the switch to
        2N, blindRotate under `key` at `limbs` (default: the first level) and extractLWEs at term 0.  Sample (j, b) of `lwes` encrypts table[phi] in its
        constant term, phi the phase the samples carry under `key`; Evaluator.packLWEs can follow.
        lwe_key (an api.LWESwitchKey of createLWESwitchKey(z)): the samples go through lweKeySwitch(to_2n=True) to dimension n = lwe_key.n and `key` is
        createBlindRotationKey(z): n CMux steps instead of N, and phi is the phase of the MESSAGE, round(2N m / t) up to the noise -- the result is f(m).
        lwe_key=None: lweModSwitch and a key of dimension N.  phi is then beta + sum_i a_i d_i for the digits d of `key` in the order of the words: with
        createBlindRotationKey(kg.extractionSecret()) that is the message's phase too; with the default createBlindRotationKey() (digit i = s_i) it is
        not, because extraction leaves c1 as a polynomial whose word i multiplies -s_(N-i)."""
        ev, ctx = evaluator, self.context
        limbs = int(limbs or ctx.first_limbs)
        if lwe_key is not None and (not isinstance(lwe_key, api.LWESwitchKey) or lwe_key.n != key.n):
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "LookupTable: the LWE switching key and the blind rotation key differ in dimension")
        low = ev.modSwitchTo(ct_batch, 1) if ct_batch.limbs > 1 else ct_batch
        lwes = ev.extractLWEs(low, terms)
        samples = ev.lweModSwitch(lwes) if lwe_key is None else ev.lweKeySwitch(lwes, lwe_key, to_2n=True, scratch_limit_words=scratch_limit_words)
        rotated = ev.blindRotate(samples, key, self.test_vector(limbs), limbs=limbs, scratch_limit_words=scratch_limit_words)
        return rotated, ev.extractLWEs(rotated, [0])
