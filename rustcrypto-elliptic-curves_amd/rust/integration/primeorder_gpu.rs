//! UNBUILT SOURCE.  Layer 2 of the Rust side for the primeorder curves (P-256, P-384): a module a maintainer would add
//! as `primeorder/src/gpu.rs` (inside the crate: `ProjectivePoint<C>`'s coordinates are `pub(crate)`).
//!
//! Coordinates travel as canonical big-endian bytes, `PrimeField::to_repr` of `C::FieldElement` (for these curves that
//! leaves the Montgomery domain first: p256 field.rs:281-284, fiat_p384_from_montgomery); scalars as `to_repr` too
//! (p384's `Scalar` is in Montgomery form internally, scalar.rs:335-339 - `to_repr` canonicalises it).
use alloc::vec::Vec;
use ecgpu_sys::{Context, Error, ECGPU_EXACT_REFERENCE, ECGPU_H2C_NU, ECGPU_H2C_RO, ECGPU_P256, ECGPU_P384, ECGPU_PT_AFFINE, ECGPU_PT_PROJECTIVE};
use elliptic_curve::{ff::PrimeField, FieldBytes, Scalar};

use crate::{AffinePoint, PrimeCurveParams, ProjectivePoint};

/// The library's curve id for a `PrimeCurveParams` implementor.
pub trait GpuCurve: PrimeCurveParams {
    const ECGPU_ID: i32;
}
// in p256 / p384:   impl primeorder::gpu::GpuCurve for NistP256 { const ECGPU_ID: i32 = ECGPU_P256; }
//                   impl primeorder::gpu::GpuCurve for NistP384 { const ECGPU_ID: i32 = ECGPU_P384; }
const _: (i32, i32) = (ECGPU_P256, ECGPU_P384);

fn nb<C: GpuCurve>() -> usize { Context::field_bytes(C::ECGPU_ID) }
fn put_projective<C: GpuCurve>(buf: &mut Vec<u8>, p: &ProjectivePoint<C>) {
    buf.extend_from_slice(p.x.to_repr().as_ref());
    buf.extend_from_slice(p.y.to_repr().as_ref());
    buf.extend_from_slice(p.z.to_repr().as_ref());
}
fn get_field<C: GpuCurve>(b: &[u8]) -> C::FieldElement {
    C::FieldElement::from_repr(FieldBytes::<C>::clone_from_slice(b)).unwrap()      // canonical by construction
}
fn get_projective<C: GpuCurve>(b: &[u8]) -> ProjectivePoint<C> {
    let n = nb::<C>();
    ProjectivePoint { x: get_field::<C>(&b[..n]), y: get_field::<C>(&b[n..2 * n]), z: get_field::<C>(&b[2 * n..3 * n]) }
}
fn get_affine<C: GpuCurve>(xy: &[u8], infinity: u8) -> AffinePoint<C> {
    let n = nb::<C>();
    if infinity != 0 { AffinePoint::IDENTITY } else { AffinePoint { x: get_field::<C>(&xy[..n]), y: get_field::<C>(&xy[n..2 * n]), infinity: 0 } }
}
fn put_scalars<'a, C: GpuCurve>(it: impl Iterator<Item = &'a Scalar<C>>) -> Vec<u8> {
    let mut v = Vec::new();
    for k in it { v.extend_from_slice(k.to_repr().as_ref()); }
    v
}

/// Bulk `MulByGenerator::mul_by_generator` (projective.rs:422-431, "TODO: precomputed basepoint tables" - the device has
/// them): throughput schedule for PUBLIC scalars, affine results.
pub fn mul_by_generator_batch<C: GpuCurve>(gpu: &Context, scalars: &[Scalar<C>]) -> Result<Vec<AffinePoint<C>>, Error> {
    let s = put_scalars::<C>(scalars.iter());
    let (out, inf, _) = gpu.lincomb(C::ECGPU_ID, &s, None, ECGPU_PT_AFFINE, 1, ECGPU_PT_AFFINE, 0, false)?;
    Ok(out.chunks_exact(2 * nb::<C>()).zip(inf.iter()).map(|(xy, i)| get_affine::<C>(xy, *i)).collect())
}

/// Bulk `ProjectivePoint::mul` (projective.rs:106-150) exactly as the CPU path computes it - same (X, Y, Z), constant-time
/// 15-way table scans - for secret scalars (ECDH, nonces).
pub fn mul_exact_batch<C: GpuCurve>(gpu: &Context, points: &[ProjectivePoint<C>], scalars: &[Scalar<C>]) -> Result<Vec<ProjectivePoint<C>>, Error> {
    assert_eq!(points.len(), scalars.len());
    let s = put_scalars::<C>(scalars.iter());
    let mut p = Vec::with_capacity(3 * nb::<C>() * points.len());
    for q in points { put_projective::<C>(&mut p, q); }
    let (out, _, _) = gpu.lincomb(C::ECGPU_ID, &s, Some(&p), ECGPU_PT_PROJECTIVE, 1, ECGPU_PT_PROJECTIVE, ECGPU_EXACT_REFERENCE, false)?;
    Ok(out.chunks_exact(3 * nb::<C>()).map(get_projective::<C>).collect())
}

/// The default `LinearCombination::lincomb` (x * k + y * l, projective.rs:415-420) for many independent pairs.
pub fn lincomb_batch<C: GpuCurve>(gpu: &Context, terms: &[[(ProjectivePoint<C>, Scalar<C>); 2]]) -> Result<Vec<AffinePoint<C>>, Error> {
    let s = put_scalars::<C>(terms.iter().flat_map(|t| t.iter().map(|(_, k)| k)));
    let mut p = Vec::with_capacity(6 * nb::<C>() * terms.len());
    for t in terms { for (q, _) in t { put_projective::<C>(&mut p, q); } }
    let (out, inf, _) = gpu.lincomb(C::ECGPU_ID, &s, Some(&p), ECGPU_PT_PROJECTIVE, 2, ECGPU_PT_AFFINE, 0, false)?;
    Ok(out.chunks_exact(2 * nb::<C>()).zip(inf.iter()).map(|(xy, i)| get_affine::<C>(xy, *i)).collect())
}

/// `BatchNormalize<[ProjectivePoint<C>]>::batch_normalize` (projective.rs:363-379).
pub fn batch_normalize_gpu<C: GpuCurve>(gpu: &Context, points: &[ProjectivePoint<C>]) -> Result<Vec<AffinePoint<C>>, Error> {
    let mut p = Vec::with_capacity(3 * nb::<C>() * points.len());
    for q in points { put_projective::<C>(&mut p, q); }
    let (xy, inf) = gpu.batch_normalize(C::ECGPU_ID, &p)?;
    Ok(xy.chunks_exact(2 * nb::<C>()).zip(inf.iter()).map(|(c, i)| get_affine::<C>(c, *i)).collect())
}

/// `ProjectivePoint<C>: ConstantTimeEq` (projective.rs:191-198, equality of the affine forms) for many pairs.
pub fn eq_batch<C: GpuCurve>(gpu: &Context, a: &[ProjectivePoint<C>], b: &[ProjectivePoint<C>]) -> Result<Vec<bool>, Error> {
    assert_eq!(a.len(), b.len());
    let (mut pa, mut pb) = (Vec::new(), Vec::new());
    for q in a { put_projective::<C>(&mut pa, q); }
    for q in b { put_projective::<C>(&mut pb, q); }
    Ok(gpu.point_eq(C::ECGPU_ID, &pa, &pb)?.into_iter().map(|f| f != 0).collect())
}

/// `GroupDigest` for many messages under one DST (p256 | p384 src/arithmetic/hash2curve.rs; the trait's methods take
/// `&[&[u8]]` message parts and DST parts: concatenate them first).  SHA-2, expand_message_xmd, FromOkm, the maps and their
/// sum all run on the device.
pub fn hash_from_bytes_batch<C: GpuCurve>(gpu: &Context, msgs: &[&[u8]], dst: &[u8]) -> Result<Vec<AffinePoint<C>>, Error> {
    let (xy, inf) = gpu.hash_to_curve(C::ECGPU_ID, msgs, dst, ECGPU_H2C_RO)?;
    Ok(xy.chunks_exact(2 * nb::<C>()).zip(inf.iter()).map(|(c, i)| get_affine::<C>(c, *i)).collect())
}
/// `GroupDigest::encode_from_bytes` (the nonuniform encoding: one map per message).
pub fn encode_from_bytes_batch<C: GpuCurve>(gpu: &Context, msgs: &[&[u8]], dst: &[u8]) -> Result<Vec<AffinePoint<C>>, Error> {
    let (xy, inf) = gpu.hash_to_curve(C::ECGPU_ID, msgs, dst, ECGPU_H2C_NU)?;
    Ok(xy.chunks_exact(2 * nb::<C>()).zip(inf.iter()).map(|(c, i)| get_affine::<C>(c, *i)).collect())
}
/// `GroupDigest::hash_to_scalar` (VOPRF DeriveKeyPair and friends: the results may be secret keys).
pub fn hash_to_scalar_batch<C: GpuCurve>(gpu: &Context, msgs: &[&[u8]], dst: &[u8]) -> Result<Vec<Scalar<C>>, Error> {
    let out = gpu.hash_to_scalar(C::ECGPU_ID, msgs, dst)?;
    // the library only returns canonical scalars: from_repr cannot fail on them
    Ok(out.chunks_exact(nb::<C>()).map(|b| Scalar::<C>::from_repr(FieldBytes::<C>::clone_from_slice(b)).unwrap()).collect())
}

/// `PrehashSigner<Signature<C>>::sign_prehash` of `ecdsa::SigningKey<C>` (p256/src/ecdsa.rs:120-134, p384/src/ecdsa.rs:114-128) for many
/// (key, digest) pairs: RFC 6979 nonces on the curve's digest (HMAC-DRBG over SHA-256 / SHA-384), k G on the constant-time kernel,
/// s = k^-1 (z + r d), all on the device.  `digests`: after bits2field (field-sized).  None where the reference returns Err.
pub fn ecdsa_sign_prehash_batch<C: GpuCurve>(gpu: &Context, keys: &[Scalar<C>], digests: &[FieldBytes<C>]) -> Result<Vec<Option<(Vec<u8>, u8)>>, Error> {
    ecdsa_sign_prehash_with(gpu, keys, digests, None)
}
/// `RandomizedPrehashSigner::sign_prehash_with_rng`: the same with field-sized additional data per signature, drawn by the caller
/// from its `CryptoRngCore` (the reference fills `ad` the same way before `try_sign_prehashed_rfc6979`).
pub fn ecdsa_sign_prehash_randomized_batch<C: GpuCurve>(gpu: &Context, keys: &[Scalar<C>], digests: &[FieldBytes<C>], added: &[FieldBytes<C>]) -> Result<Vec<Option<(Vec<u8>, u8)>>, Error> {
    assert_eq!(added.len(), keys.len());
    ecdsa_sign_prehash_with(gpu, keys, digests, Some(added))
}
fn ecdsa_sign_prehash_with<C: GpuCurve>(gpu: &Context, keys: &[Scalar<C>], digests: &[FieldBytes<C>], added: Option<&[FieldBytes<C>]>) -> Result<Vec<Option<(Vec<u8>, u8)>>, Error> {
    assert_eq!(keys.len(), digests.len());
    let flat = |v: &[FieldBytes<C>]| { let mut o = Vec::with_capacity(nb::<C>() * v.len()); for b in v { o.extend_from_slice(b.as_ref()); } o };
    let ad = added.map(flat);
    let (sig, rec, ok) = gpu.ecdsa_sign_prehash(C::ECGPU_ID, &put_scalars::<C>(keys.iter()), &flat(digests), ad.as_deref(), 0)?;
    Ok(sig.chunks_exact(2 * nb::<C>()).zip(rec.iter().zip(ok.iter())).map(|(s, (r, k))| if *k != 0 { Some((s.to_vec(), *r)) } else { None }).collect())
}

/// `Signer<Signature<C>>::sign` of `ecdsa::SigningKey<C>` for many (key, message) pairs: the curve's own digest (SHA-256 for P-256,
/// SHA-384 for P-384) runs on the device, then everything of `ecdsa_sign_prehash_batch`.  `added`: the additional data of
/// `RandomizedSigner::sign_with_rng`.
pub fn ecdsa_sign_batch<C: GpuCurve>(gpu: &Context, keys: &[Scalar<C>], msgs: &[&[u8]], added: Option<&[FieldBytes<C>]>) -> Result<Vec<Option<(Vec<u8>, u8)>>, Error> {
    assert!(keys.len() == msgs.len() && added.map_or(true, |a| a.len() == keys.len()));
    let ad = added.map(|v| { let mut o = Vec::with_capacity(nb::<C>() * v.len()); for b in v { o.extend_from_slice(b.as_ref()); } o });
    let (sig, rec, ok) = gpu.ecdsa_sign_msg(C::ECGPU_ID, &put_scalars::<C>(keys.iter()), msgs, ad.as_deref(), 0)?;
    Ok(sig.chunks_exact(2 * nb::<C>()).zip(rec.iter().zip(ok.iter())).map(|(s, (r, k))| if *k != 0 { Some((s.to_vec(), *r)) } else { None }).collect())
}
/// `Verifier<Signature<C>>::verify` of `ecdsa::VerifyingKey<C>` for many (message, r || s, x || y) triples, all flat big-endian bytes.
pub fn ecdsa_verify_batch<C: GpuCurve>(gpu: &Context, msgs: &[&[u8]], sigs_rs: &[u8], pubkeys_xy: &[u8]) -> Result<Vec<bool>, Error> {
    Ok(gpu.ecdsa_verify_msg(C::ECGPU_ID, msgs, sigs_rs, pubkeys_xy, 0)?.into_iter().map(|f| f != 0).collect())
}
/// `VerifyingKey::<C>::recover_from_msg` -> x || y of each key, None where the reference returns Err.
pub fn ecdsa_recover_from_msg_batch<C: GpuCurve>(gpu: &Context, msgs: &[&[u8]], sigs_rs: &[u8], recovery_ids: &[u8]) -> Result<Vec<Option<Vec<u8>>>, Error> {
    let (xy, ok) = gpu.ecdsa_recover_msg(C::ECGPU_ID, msgs, sigs_rs, recovery_ids, 0)?;
    Ok(xy.chunks_exact(2 * nb::<C>()).zip(ok.iter()).map(|(p, k)| if *k != 0 { Some(p.to_vec()) } else { None }).collect())
}
