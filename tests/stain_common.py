"""What the stain-normalisation tests share: a generator of synthetic H&E tiles and a transcription of the published Macenko script
(the ``normalizeStaining`` that torchstain / staintools / HistomicsTK restate) to pin the project's oracle against."""
import numpy as np

from plip_amd import preprocess as PP

# a source stain matrix unlike the target (columns: haematoxylin, eosin), unit columns
HE_SOURCE = np.array([[0.65, 0.07], [0.70, 0.99], [0.29, 0.11]])
HE_SOURCE = HE_SOURCE / np.sqrt((HE_SOURCE ** 2).sum(axis=0))


def he_tile(seed: int, h: int = 64, w: int = 64, glass: float = 0.3, he=None, strength=(1.0, 1.0)) -> np.ndarray:
    """uint8 [h,w,3]: two gamma-distributed concentrations through ``he`` (default HE_SOURCE), Gaussian noise on the optical density,
    about ``glass`` of the pixels near white; written to bytes by the inverse of the oracle's lookup (Io 240)."""
    rng = np.random.default_rng([20260, seed])
    he = HE_SOURCE if he is None else np.asarray(he, np.float64)
    n = h * w
    conc = np.stack([rng.gamma(2.0, 0.45 * strength[0], n), rng.gamma(2.5, 0.30 * strength[1], n)])      # [2, n]
    od = (he @ conc).T + rng.normal(0.0, 0.02, (n, 3))
    is_glass = rng.random(n) < glass
    # (glass a shade under Io: a pixel of three bytes Io - 1 has C = 0 and an output of exactly Io, an integer by construction, which
    # the GPU tests' census of "bytes that rounding could move" would count)
    od[is_glass] = 0.01 + np.abs(rng.normal(0.0, 0.02, (int(is_glass.sum()), 3)))
    px = np.clip(np.rint(240.0 * np.exp(-od) - 1.0), 0, 255).astype(np.uint8)
    return px.reshape(h, w, 3)


def glass_tile(seed: int, h: int = 64, w: int = 64) -> np.ndarray:
    """uint8 [h,w,3] without tissue: every byte's optical density is below the default beta"""
    return np.random.default_rng([20261, seed]).integers(225, 256, (h, w, 3), dtype=np.uint8)


def published_macenko(img: np.ndarray, Io=240, alpha=1, beta=0.15, HERef=None, maxCRef=None):
    """The canonical script, line for line (np.cov, eigh, np.percentile, lstsq, clip at 255) -> (normalised uint8, HE [3,2], maxC [2])."""
    HERef = PP.HE_REF if HERef is None else HERef
    maxCRef = PP.MAXC_REF if maxCRef is None else maxCRef
    h, w, _ = img.shape
    img = img.reshape((-1, 3))
    OD = -np.log((img.astype(np.float64) + 1) / Io)
    ODhat = OD[~np.any(OD < beta, axis=1)]
    eigvals, eigvecs = np.linalg.eigh(np.cov(ODhat.T))
    That = ODhat.dot(eigvecs[:, 1:3])
    phi = np.arctan2(That[:, 1], That[:, 0])
    minPhi = np.percentile(phi, alpha)
    maxPhi = np.percentile(phi, 100 - alpha)
    vMin = eigvecs[:, 1:3].dot(np.array([(np.cos(minPhi), np.sin(minPhi))]).T)
    vMax = eigvecs[:, 1:3].dot(np.array([(np.cos(maxPhi), np.sin(maxPhi))]).T)
    if vMin[0] > vMax[0]:
        HE = np.array((vMin[:, 0], vMax[:, 0])).T
    else:
        HE = np.array((vMax[:, 0], vMin[:, 0])).T
    Y = np.reshape(OD, (-1, 3)).T
    C = np.linalg.lstsq(HE, Y, rcond=None)[0]
    maxC = np.array([np.percentile(C[0, :], 99), np.percentile(C[1, :], 99)])
    tmp = np.divide(maxC, maxCRef)
    C2 = np.divide(C, tmp[:, np.newaxis])
    Inorm = np.multiply(Io, np.exp(-HERef.dot(C2)))
    Inorm[Inorm > 255] = 255                                     # (the script writes 254 here in some copies; the issue's is 255)
    Inorm = np.reshape(Inorm.T, (h, w, 3)).astype(np.uint8)
    return Inorm, HE, maxC
