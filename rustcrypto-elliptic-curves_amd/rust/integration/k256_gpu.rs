//! UNBUILT SOURCE.  Layer 2 of the Rust side for secp256k1: a module a maintainer would add as
//! `k256/src/arithmetic/gpu.rs` (inside the crate: it reads the private coordinates of `ProjectivePoint`).
//! Bulk, trait-shaped entry points over the reference's own types, backed by `ecgpu_sys::Context`.
//!
//! Wire format = what the reference's own serialisers produce: `FieldElement::to_bytes` after `normalize`
//! (field.rs:118-120, field_5x52.rs:96-131), `Scalar::to_bytes` (scalar.rs:94-96); nothing here depends on the in-memory
//! layout of the types (which is not ABI-stable, field_impl.rs:23-28).
use alloc::vec::Vec;
use ecgpu_sys::{Context, Error, Group, ECGPU_EXACT_REFERENCE, ECGPU_H2C_NU, ECGPU_H2C_RO, ECGPU_K256, ECGPU_PT_AFFINE, ECGPU_PT_PROJECTIVE, ECGPU_SC_INV};
use elliptic_curve::{ff::PrimeField, subtle::{Choice, CtOption}};

use crate::{AffinePoint, FieldBytes, ProjectivePoint, Scalar};
use super::FieldElement;

fn put_projective(buf: &mut Vec<u8>, p: &ProjectivePoint) {
    buf.extend_from_slice(&p.x.normalize().to_bytes());
    buf.extend_from_slice(&p.y.normalize().to_bytes());
    buf.extend_from_slice(&p.z.normalize().to_bytes());
}
fn get_field(b: &[u8]) -> FieldElement {
    // the library only ever returns canonical values (< p): from_bytes cannot fail on them
    FieldElement::from_bytes(FieldBytes::from_slice(b)).unwrap()
}
fn get_projective(b: &[u8]) -> ProjectivePoint {
    ProjectivePoint { x: get_field(&b[..32]), y: get_field(&b[32..64]), z: get_field(&b[64..96]) }
}
fn get_affine(xy: &[u8], infinity: u8) -> AffinePoint {
    if infinity != 0 { AffinePoint::IDENTITY } else { AffinePoint { x: get_field(&xy[..32]), y: get_field(&xy[32..64]), infinity: 0 } }
}
fn put_scalars<'a>(it: impl Iterator<Item = &'a Scalar>) -> Vec<u8> {
    let mut v = Vec::new();
    for k in it { v.extend_from_slice(&k.to_bytes()); }
    v
}

/// Bulk `Scalar::invert` (scalar.rs:161-209): one `CtOption` per scalar, none for 0 as on the CPU path.  Constant-time
/// kernel (csrc/scalar_ops.hpp: a lane shares one Fermat inversion over its batch with masks, no branch on a value), so it
/// serves `invert_vartime` callers as well.
pub fn invert_batch(gpu: &Context, scalars: &[Scalar]) -> Result<Vec<CtOption<Scalar>>, Error> {
    let s = put_scalars(scalars.iter());
    let (out, ok) = gpu.scalar_op(ECGPU_K256, ECGPU_SC_INV, &s, None)?;
    Ok(out
        .chunks_exact(32)
        .zip(ok.iter())
        .map(|(b, &k)| {
            // the library only returns canonical scalars: from_repr cannot fail on them
            let v = Scalar::from_repr(*FieldBytes::from_slice(b)).unwrap();
            CtOption::new(v, Choice::from(k))
        })
        .collect())
}

/// Bulk `MulByGenerator::mul_by_generator` (mul.rs:415-440): out[i] = scalars[i] * G, the exact (X, Y, Z) the CPU path
/// returns (constant-time schedule: the scalars may be secret).
pub fn mul_by_generator_batch(gpu: &Context, scalars: &[Scalar]) -> Result<Vec<ProjectivePoint>, Error> {
    let s = put_scalars(scalars.iter());
    let (out, _, _) = gpu.lincomb(ECGPU_K256, &s, None, ECGPU_PT_AFFINE, 1, ECGPU_PT_PROJECTIVE, ECGPU_EXACT_REFERENCE, false)?;
    Ok(out.chunks_exact(96).map(get_projective).collect())
}

/// Bulk `&ProjectivePoint * &Scalar` (mul.rs:442-481) on PUBLIC data, throughput schedule: the group elements as affine
/// points (use `flags = ECGPU_EXACT_REFERENCE` through `Context::lincomb` for secret scalars or exact triples).
pub fn mul_batch(gpu: &Context, points: &[ProjectivePoint], scalars: &[Scalar]) -> Result<Vec<AffinePoint>, Error> {
    assert_eq!(points.len(), scalars.len());
    let s = put_scalars(scalars.iter());
    let mut p = Vec::with_capacity(96 * points.len());
    for q in points { put_projective(&mut p, q); }
    let (out, inf, _) = gpu.lincomb(ECGPU_K256, &s, Some(&p), ECGPU_PT_PROJECTIVE, 1, ECGPU_PT_AFFINE, 0, false)?;
    Ok(out.chunks_exact(64).zip(inf.iter()).map(|(xy, i)| get_affine(xy, *i)).collect())
}

/// `LinearCombinationExt<[(ProjectivePoint, Scalar)]>::lincomb_ext` (mul.rs:325-340) at MSM scale: one bucket-method sum
/// over the whole slice, split over the devices of a `Group` (every device sums a contiguous range of the terms, one point per
/// device is all-gathered - RCCL over xGMI - and folded on the first device; a group of one device is the single-GPU call).
/// The group element is that of the CPU path; the representative is (x : y : 1).
pub fn lincomb_ext_gpu(gpus: &Group, points_and_scalars: &[(ProjectivePoint, Scalar)]) -> Result<ProjectivePoint, Error> {
    let s = put_scalars(points_and_scalars.iter().map(|(_, k)| k));
    let mut p = Vec::with_capacity(96 * points_and_scalars.len());
    for (q, _) in points_and_scalars { put_projective(&mut p, q); }
    let out = gpus.msm(ECGPU_K256, &s, &p, ECGPU_PT_PROJECTIVE, ECGPU_PT_PROJECTIVE)?;
    Ok(get_projective(&out))
}

/// Bulk `&ProjectivePoint * &Scalar` over a `Group`: contiguous index ranges per device, no collective.
pub fn mul_batch_group(gpus: &Group, points: &[ProjectivePoint], scalars: &[Scalar]) -> Result<Vec<AffinePoint>, Error> {
    assert_eq!(points.len(), scalars.len());
    let s = put_scalars(scalars.iter());
    let mut p = Vec::with_capacity(96 * points.len());
    for q in points { put_projective(&mut p, q); }
    let (out, inf) = gpus.lincomb(ECGPU_K256, &s, Some(&p), ECGPU_PT_PROJECTIVE, 1, ECGPU_PT_AFFINE, 0)?;
    Ok(out.chunks_exact(64).zip(inf.iter()).map(|(xy, i)| get_affine(xy, *i)).collect())
}

/// `LinearCombination::lincomb(x, k, y, l)` (mul.rs:313-323) for many independent pairs: out[i] = x_i k_i + y_i l_i.
pub fn lincomb_batch(gpu: &Context, terms: &[[(ProjectivePoint, Scalar); 2]]) -> Result<Vec<AffinePoint>, Error> {
    let s = put_scalars(terms.iter().flat_map(|t| t.iter().map(|(_, k)| k)));
    let mut p = Vec::with_capacity(192 * terms.len());
    for t in terms { for (q, _) in t { put_projective(&mut p, q); } }
    let (out, inf, _) = gpu.lincomb(ECGPU_K256, &s, Some(&p), ECGPU_PT_PROJECTIVE, 2, ECGPU_PT_AFFINE, 0, false)?;
    Ok(out.chunks_exact(64).zip(inf.iter()).map(|(xy, i)| get_affine(xy, *i)).collect())
}

/// `BatchNormalize<[ProjectivePoint]>::batch_normalize` (projective.rs:337-348): one shared inversion per 16 points on
/// the device instead of one `BatchInvert` over the slice; identities come back as `AffinePoint::IDENTITY` (:361-364).
pub fn batch_normalize_gpu(gpu: &Context, points: &[ProjectivePoint]) -> Result<Vec<AffinePoint>, Error> {
    let mut p = Vec::with_capacity(96 * points.len());
    for q in points { put_projective(&mut p, q); }
    let (xy, inf) = gpu.batch_normalize(ECGPU_K256, &p)?;
    Ok(xy.chunks_exact(64).zip(inf.iter()).map(|(c, i)| get_affine(c, *i)).collect())
}

/// `ProjectivePoint::ct_eq` (projective.rs:421-446) for many pairs.
pub fn eq_batch(gpu: &Context, a: &[ProjectivePoint], b: &[ProjectivePoint]) -> Result<Vec<bool>, Error> {
    assert_eq!(a.len(), b.len());
    let (mut pa, mut pb) = (Vec::with_capacity(96 * a.len()), Vec::with_capacity(96 * b.len()));
    for q in a { put_projective(&mut pa, q); }
    for q in b { put_projective(&mut pb, q); }
    Ok(gpu.point_eq(ECGPU_K256, &pa, &pb)?.into_iter().map(|f| f != 0).collect())
}

/// `GroupDigest` for many messages under one DST (arithmetic/hash2curve.rs; the trait's methods take `&[&[u8]]` message
/// parts and DST parts: concatenate them first).  SHA-256, expand_message_xmd, FromOkm, the two maps with their isogeny
/// and the sum all run on the device.
pub fn hash_from_bytes_batch(gpu: &Context, msgs: &[&[u8]], dst: &[u8]) -> Result<Vec<AffinePoint>, Error> {
    let (xy, inf) = gpu.hash_to_curve(ECGPU_K256, msgs, dst, ECGPU_H2C_RO)?;
    Ok(xy.chunks_exact(64).zip(inf.iter()).map(|(c, i)| get_affine(c, *i)).collect())
}
/// `GroupDigest::encode_from_bytes` (the nonuniform encoding: one map per message).
pub fn encode_from_bytes_batch(gpu: &Context, msgs: &[&[u8]], dst: &[u8]) -> Result<Vec<AffinePoint>, Error> {
    let (xy, inf) = gpu.hash_to_curve(ECGPU_K256, msgs, dst, ECGPU_H2C_NU)?;
    Ok(xy.chunks_exact(64).zip(inf.iter()).map(|(c, i)| get_affine(c, *i)).collect())
}
/// `GroupDigest::hash_to_scalar`.
pub fn hash_to_scalar_batch(gpu: &Context, msgs: &[&[u8]], dst: &[u8]) -> Result<Vec<Scalar>, Error> {
    let out = gpu.hash_to_scalar(ECGPU_K256, msgs, dst)?;
    // the library only returns canonical scalars: from_repr cannot fail on them
    Ok(out.chunks_exact(32).map(|b| Scalar::from_repr(*FieldBytes::from_slice(b)).unwrap()).collect())
}
/// BIP340 `VerifyingKey::verify_prehash` (schnorr/verifying.rs:62-93) for many (key, digest, signature) triples: the tagged
/// challenge hash runs on the device as well.
pub fn schnorr_verify_prehash_batch(gpu: &Context, pubkeys_x: &[[u8; 32]], prehashes: &[[u8; 32]], sigs: &[[u8; 64]]) -> Result<Vec<bool>, Error> {
    assert!(pubkeys_x.len() == prehashes.len() && prehashes.len() == sigs.len());
    let ok = gpu.schnorr_verify_prehash(&pubkeys_x.concat(), &sigs.concat(), &prehashes.concat())?;
    Ok(ok.into_iter().map(|f| f != 0).collect())
}
/// The same answers from BIP340's batch equation (one multi-scalar multiplication over 2n + 1 terms; the per-signature pipeline
/// runs only for a batch that holds an invalid signature) -> (per-signature flags, all valid).  The library draws the seed of the
/// equation's coefficients itself.
pub fn schnorr_batch_verify_prehash(gpu: &Context, pubkeys_x: &[[u8; 32]], prehashes: &[[u8; 32]], sigs: &[[u8; 64]]) -> Result<(Vec<bool>, bool), Error> {
    assert!(pubkeys_x.len() == prehashes.len() && prehashes.len() == sigs.len());
    let (ok, all_valid) = gpu.schnorr_batch_verify_prehash(&pubkeys_x.concat(), &sigs.concat(), &prehashes.concat(), None, 0)?;
    Ok((ok.into_iter().map(|f| f != 0).collect(), all_valid))
}

/// `PrehashSigner<Signature>::sign_prehash` of `ecdsa::SigningKey<Secp256k1>` for many (key, digest) pairs: RFC 6979 nonces
/// (HMAC-DRBG on SHA-256), k G on the constant-time kernel, low-s normalisation as ecdsa.rs:182-196.  `digests`: after bits2field
/// (32 bytes).  None where the reference returns Err.
pub fn ecdsa_sign_prehash_batch(gpu: &Context, keys: &[Scalar], digests: &[[u8; 32]]) -> Result<Vec<Option<([u8; 64], u8)>>, Error> {
    assert_eq!(keys.len(), digests.len());
    let (sig, rec, ok) = gpu.ecdsa_sign_prehash(ECGPU_K256, &put_scalars(keys.iter()), &digests.concat(), None, ecgpu_sys::ECGPU_ECDSA_LOW_S)?;
    Ok(sig.chunks_exact(64).zip(rec.iter().zip(ok.iter())).map(|(s, (r, k))| if *k != 0 { Some((s.try_into().unwrap(), *r)) } else { None }).collect())
}
/// `RandomizedPrehashSigner::sign_prehash_with_rng`: the same with 32 bytes of additional data per signature, drawn by the caller
/// from its `CryptoRngCore` (the reference fills `ad` the same way before `try_sign_prehashed_rfc6979`).
pub fn ecdsa_sign_prehash_randomized_batch(gpu: &Context, keys: &[Scalar], digests: &[[u8; 32]], added: &[[u8; 32]]) -> Result<Vec<Option<([u8; 64], u8)>>, Error> {
    assert!(keys.len() == digests.len() && digests.len() == added.len());
    let (sig, rec, ok) = gpu.ecdsa_sign_prehash(ECGPU_K256, &put_scalars(keys.iter()), &digests.concat(), Some(&added.concat()), ecgpu_sys::ECGPU_ECDSA_LOW_S)?;
    Ok(sig.chunks_exact(64).zip(rec.iter().zip(ok.iter())).map(|(s, (r, k))| if *k != 0 { Some((s.try_into().unwrap(), *r)) } else { None }).collect())
}
/// BIP340 `schnorr::SigningKey::sign_prehash_with_aux_rand` (schnorr/signing.rs:79-120) for many (key, digest, aux_rand) triples:
/// both generator multiplications, the three tagged hashes and the arithmetic mod n run on the device.  `secret_keys`: the
/// `NonZeroScalar` bytes of the keys (the call recomputes each verifying key; no key pair is cached).  -> (signature, x-only key)
pub fn schnorr_sign_prehash_batch(gpu: &Context, secret_keys: &[[u8; 32]], prehashes: &[[u8; 32]], aux_rands: &[[u8; 32]]) -> Result<Vec<Option<([u8; 64], [u8; 32])>>, Error> {
    assert!(secret_keys.len() == prehashes.len() && prehashes.len() == aux_rands.len());
    let (sig, px, ok) = gpu.schnorr_sign_prehash(&secret_keys.concat(), &prehashes.concat(), &aux_rands.concat())?;
    Ok(sig.chunks_exact(64).zip(px.chunks_exact(32)).zip(ok.iter())
        .map(|((s, p), k)| if *k != 0 { Some((s.try_into().unwrap(), p.try_into().unwrap())) } else { None }).collect())
}

/// `Signer<Signature>::sign` of `ecdsa::SigningKey<Secp256k1>` for many (key, message) pairs: SHA-256 of each message runs on the
/// device, then everything of `ecdsa_sign_prehash_batch`.  `added`: the additional data of `RandomizedSigner::sign_with_rng`.
pub fn ecdsa_sign_batch(gpu: &Context, keys: &[Scalar], msgs: &[&[u8]], added: Option<&[[u8; 32]]>) -> Result<Vec<Option<([u8; 64], u8)>>, Error> {
    assert!(keys.len() == msgs.len() && added.map_or(true, |a| a.len() == keys.len()));
    let ad = added.map(|a| a.concat());
    let (sig, rec, ok) = gpu.ecdsa_sign_msg(ECGPU_K256, &put_scalars(keys.iter()), msgs, ad.as_deref(), ecgpu_sys::ECGPU_ECDSA_LOW_S)?;
    Ok(sig.chunks_exact(64).zip(rec.iter().zip(ok.iter())).map(|(s, (r, k))| if *k != 0 { Some((s.try_into().unwrap(), *r)) } else { None }).collect())
}
/// `Verifier<Signature>::verify` of `ecdsa::VerifyingKey<Secp256k1>` for many (message, r || s, x || y) triples (low-s rule as
/// ecdsa.rs:198-207).
pub fn ecdsa_verify_batch(gpu: &Context, msgs: &[&[u8]], sigs: &[[u8; 64]], pubkeys_xy: &[[u8; 64]]) -> Result<Vec<bool>, Error> {
    assert!(msgs.len() == sigs.len() && sigs.len() == pubkeys_xy.len());
    let ok = gpu.ecdsa_verify_msg(ECGPU_K256, msgs, &sigs.concat(), &pubkeys_xy.concat(), ecgpu_sys::ECGPU_ECDSA_LOW_S)?;
    Ok(ok.into_iter().map(|f| f != 0).collect())
}
/// `VerifyingKey::recover_from_msg` (exercised by ecdsa.rs:259-336) -> x || y of each key, None where the reference returns Err.
pub fn ecdsa_recover_from_msg_batch(gpu: &Context, msgs: &[&[u8]], sigs: &[[u8; 64]], recovery_ids: &[u8]) -> Result<Vec<Option<[u8; 64]>>, Error> {
    assert!(msgs.len() == sigs.len() && sigs.len() == recovery_ids.len());
    let (xy, ok) = gpu.ecdsa_recover_msg(ECGPU_K256, msgs, &sigs.concat(), recovery_ids, ecgpu_sys::ECGPU_ECDSA_LOW_S)?;
    Ok(xy.chunks_exact(64).zip(ok.iter()).map(|(p, k)| if *k != 0 { Some(p.try_into().unwrap()) } else { None }).collect())
}
/// The Ethereum shape of ecdsa.rs:84-143 for a batch, `signing_key.sign_digest_recoverable(Keccak256::new_with_prefix(msg))`: Keccak-256
/// of each message runs on the device, the RFC 6979 nonce stays on HMAC-SHA-256.  `added`: the additional data of
/// `RandomizedDigestSigner::sign_digest_with_rng`.  -> (signature, recovery id)
pub fn ecdsa_sign_keccak256_batch(gpu: &Context, keys: &[Scalar], msgs: &[&[u8]], added: Option<&[[u8; 32]]>) -> Result<Vec<Option<([u8; 64], u8)>>, Error> {
    assert!(keys.len() == msgs.len() && added.map_or(true, |a| a.len() == keys.len()));
    let ad = added.map(|a| a.concat());
    let (sig, rec, ok) = gpu.ecdsa_sign_digest(ECGPU_K256, ecgpu_sys::ECGPU_KECCAK256, &put_scalars(keys.iter()), msgs, ad.as_deref(), ecgpu_sys::ECGPU_ECDSA_LOW_S)?;
    Ok(sig.chunks_exact(64).zip(rec.iter().zip(ok.iter())).map(|(s, (r, k))| if *k != 0 { Some((s.try_into().unwrap(), *r)) } else { None }).collect())
}
/// `verifying_key.verify_digest(Keccak256::new_with_prefix(msg), &sig)` for many (message, r || s, x || y) triples
pub fn ecdsa_verify_keccak256_batch(gpu: &Context, msgs: &[&[u8]], sigs: &[[u8; 64]], pubkeys_xy: &[[u8; 64]]) -> Result<Vec<bool>, Error> {
    assert!(msgs.len() == sigs.len() && sigs.len() == pubkeys_xy.len());
    let ok = gpu.ecdsa_verify_digest(ECGPU_K256, ecgpu_sys::ECGPU_KECCAK256, msgs, &sigs.concat(), &pubkeys_xy.concat(), ecgpu_sys::ECGPU_ECDSA_LOW_S)?;
    Ok(ok.into_iter().map(|f| f != 0).collect())
}
/// `VerifyingKey::recover_from_digest(Keccak256::new_with_prefix(msg), &sig, recid)` (ecdsa.rs:111-143) -> x || y of each key, None
/// where the reference returns Err.  The Ethereum address of a key is the last 20 bytes of `Context::digest(ECGPU_KECCAK256, ..)` over x || y.
pub fn ecdsa_recover_keccak256_batch(gpu: &Context, msgs: &[&[u8]], sigs: &[[u8; 64]], recovery_ids: &[u8]) -> Result<Vec<Option<[u8; 64]>>, Error> {
    assert!(msgs.len() == sigs.len() && sigs.len() == recovery_ids.len());
    let (xy, ok) = gpu.ecdsa_recover_digest(ECGPU_K256, ecgpu_sys::ECGPU_KECCAK256, msgs, &sigs.concat(), recovery_ids, ecgpu_sys::ECGPU_ECDSA_LOW_S)?;
    Ok(xy.chunks_exact(64).zip(ok.iter()).map(|(p, k)| if *k != 0 { Some(p.try_into().unwrap()) } else { None }).collect())
}
/// `Signer<Signature>::try_sign` of `schnorr::SigningKey` (schnorr/signing.rs:214-218; `aux_rands = None`: the reference's
/// `Default::default()`) / `RandomizedSigner::try_sign_with_rng`: BIP340 over SHA256(msg), the digest computed on the device too.
pub fn schnorr_sign_batch(gpu: &Context, secret_keys: &[[u8; 32]], msgs: &[&[u8]], aux_rands: Option<&[[u8; 32]]>) -> Result<Vec<Option<([u8; 64], [u8; 32])>>, Error> {
    assert!(secret_keys.len() == msgs.len() && aux_rands.map_or(true, |a| a.len() == msgs.len()));
    let aux = aux_rands.map(|a| a.concat());
    let (sig, px, ok) = gpu.schnorr_sign_msg(&secret_keys.concat(), msgs, aux.as_deref())?;
    Ok(sig.chunks_exact(64).zip(px.chunks_exact(32)).zip(ok.iter())
        .map(|((s, p), k)| if *k != 0 { Some((s.try_into().unwrap(), p.try_into().unwrap())) } else { None }).collect())
}
/// `Verifier<Signature>::verify` of `schnorr::VerifyingKey` (schnorr/verifying.rs:94-98): `verify_prehash` over SHA256(msg).
pub fn schnorr_verify_batch(gpu: &Context, pubkeys_x: &[[u8; 32]], msgs: &[&[u8]], sigs: &[[u8; 64]]) -> Result<Vec<bool>, Error> {
    assert!(pubkeys_x.len() == msgs.len() && msgs.len() == sigs.len());
    let ok = gpu.schnorr_verify_msg(&pubkeys_x.concat(), msgs, &sigs.concat())?;
    Ok(ok.into_iter().map(|f| f != 0).collect())
}
