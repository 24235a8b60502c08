//! The batched `identifier_job_step` (core/src/object/file_identifier/
//! mod.rs:100-336) over libsdgpu: one call reads and hashes a whole batch of
//! orphan rows (`sdgpu_identify_files`, replacing the join_all of
//! FileMetadata::new, mod.rs:107-134), one groups them against the library's
//! Objects (`sdgpu_dedup_batch` with an Object index: the find_many of
//! mod.rs:168-185, the link of :189-225, the creates of :233-297).  The write
//! set then becomes one `create_many` + one batched `file_path` update
//! (core/crates/sync/src/manager.rs:62-97) instead of 4-5 queries per 100 rows.
//!
//! Ranks: row i of a step has rank `first_rank + i` -- its position in the
//! job's ascending-id order (file_identifier_job.rs:286-309), i.e. `step *
//! 100 + k` in the reference's terms.  rep[i] == rank: create an Object;
//! rep[i] & SDGPU_REP_EXISTING: connect to the existing Object `rep & 0x7fff_ffff`;
//! otherwise connect to the Object created for the row of rank rep[i].

use std::{io, marker::PhantomData, os::raw::c_char, path::PathBuf, ptr};

use sdgpu_sys as sys;

use crate::{check, cpath, Gpu};

/// One row's outcome (FileMetadata's cas_id + the Object decision).
pub enum Link {
    /// cas_id None (empty file, mod.rs:80-88) or a first sighting: new Object.
    Create,
    /// an Object that existed before the job (caller's handle, e.g. object.id).
    Existing(u32),
    /// the Object created for the row of this rank (this step or an earlier one).
    Row(u32),
    /// metadata / read failed: the row stays an orphan (mod.rs:113,127).
    Failed(io::Error),
}

pub struct IdentifiedRow {
    pub cas_id: Option<String>,
    pub link: Link,
}

/// The library-wide Object index of one job (mod.rs:168-185).  It borrows
/// its `Gpu`: sdgpu_close frees what the index points into, so the index
/// must be dropped first (include/sdgpu.h, sdgpu_close).
pub struct ObjectIndex<'g>(*mut sys::sdgpu_index, PhantomData<&'g Gpu>);
unsafe impl Send for ObjectIndex<'_> {}

impl<'g> ObjectIndex<'g> {
    pub fn new(gpu: &'g Gpu, capacity: u64) -> io::Result<Self> {
        let mut idx = ptr::null_mut();
        check(unsafe { sys::sdgpu_index_create(*gpu.ctx(), capacity, &mut idx) })?;
        Ok(ObjectIndex(idx, PhantomData))
    }
}

impl Drop for ObjectIndex<'_> {
    fn drop(&mut self) {
        unsafe { sys::sdgpu_index_destroy(self.0) };
    }
}

impl ObjectIndex<'_> {
    /// Objects that exist before the job (mod.rs:168-185): key -> object id.
    pub fn add_objects(&self, gpu: &Gpu, keys: &[u64], ids: &[u32]) -> io::Result<()> {
        if keys.is_empty() {
            return Ok(());
        }
        let ctx = gpu.ctx();
        let n = keys.len();
        let mut dk = ptr::null_mut();
        let mut dh = ptr::null_mut();
        check(unsafe { sys::sdgpu_alloc_device(*ctx, 8 * n, &mut dk) })?;
        check(unsafe { sys::sdgpu_alloc_device(*ctx, 4 * n, &mut dh) })?;
        let stream = unsafe { sys::sdgpu_stream(*ctx) };
        let rc = unsafe {
            check(sys::sdgpu_memcpy_async(*ctx, dk, keys.as_ptr().cast(), 8 * n, stream))
                .and_then(|_| check(sys::sdgpu_memcpy_async(*ctx, dh, ids.as_ptr().cast(), 4 * n, stream)))
                .and_then(|_| check(sys::sdgpu_index_add_objects_device(self.0, dk.cast(), dh.cast(),
                                                                       n as u64, 1, 0, stream)))
                .and_then(|_| check(sys::sdgpu_sync(*ctx)))
        };
        unsafe {
            sys::sdgpu_free_device(*ctx, dk);
            sys::sdgpu_free_device(*ctx, dh);
        }
        rc
    }

    // ---- a library-lifetime index (include/sdgpu.h, "ABI 6, additive") --------

    /// The Object owning each cas key, as a grouping's rep shows it (a rank, or
    /// SDGPU_REP_EXISTING | object id); `sys::SDGPU_INDEX_MISS` for none.  The
    /// watcher's create path (location/manager/watcher/utils.rs:240-275:
    /// find_first(object where file_paths.some(cas_id == X))) for one or a
    /// few keys, without the database.
    pub fn lookup(&self, keys: &[u64]) -> io::Result<Vec<u32>> {
        let mut values = vec![sys::SDGPU_INDEX_MISS; keys.len()];
        check(unsafe {
            sys::sdgpu_index_lookup(self.0, keys.as_ptr(), keys.len() as u64, values.as_mut_ptr())
        })?;
        Ok(values)
    }

    /// Removes the keys (watcher delete / update paths, utils.rs:746-765: the
    /// Object is deleted when no file_path is left).  `values` (what `lookup`
    /// returned): a key goes only while it still holds that value.  Returns
    /// how many keys were actually removed.
    pub fn remove(&self, gpu: &Gpu, keys: &[u64], values: Option<&[u32]>) -> io::Result<u32> {
        if keys.is_empty() {
            return Ok(0);
        }
        if values.map_or(false, |v| v.len() != keys.len()) {
            return Err(io::Error::from_raw_os_error(22));
        }
        let n = keys.len();
        let dk = DeviceMem::from_slice(gpu, keys)?;
        let dv = match values {
            Some(v) => Some(DeviceMem::from_slice(gpu, v)?),
            None => None,
        };
        let dr = DeviceMem::alloc(gpu, 4)?;
        let stream = unsafe { sys::sdgpu_stream(*gpu.ctx()) };
        check(unsafe {
            sys::sdgpu_index_remove_device(self.0, dk.ptr().cast(),
                                           dv.as_ref().map_or(ptr::null(), |d| d.ptr().cast()),
                                           n as u64, dr.ptr().cast(), stream)
        })?;
        dr.read_u32(gpu)
    }

    /// Removes every entry of the given Object ids (the orphan remover's
    /// deletions, core/src/object/orphan_remover.rs:57-90: it knows ids, not
    /// cas_ids).  `max_id` bounds the ids (it sizes the mark map).  Returns how
    /// many entries were removed.
    pub fn remove_objects(&self, gpu: &Gpu, ids: &[i32], max_id: u32) -> io::Result<u32> {
        if ids.is_empty() {
            return Ok(0);
        }
        let dh = DeviceMem::from_slice(gpu, ids)?;
        let dr = DeviceMem::alloc(gpu, 4)?;
        let stream = unsafe { sys::sdgpu_stream(*gpu.ctx()) };
        check(unsafe {
            sys::sdgpu_index_remove_objects_device(self.0, dh.ptr().cast(), ids.len() as u64, max_id,
                                                   dr.ptr().cast(), stream)
        })?;
        dr.read_u32(gpu)
    }

    /// The live entries as (key, value) pairs in no particular order: what a
    /// host persists at shutdown (its SDGPU_REP_EXISTING entries go back in
    /// with `add_objects` at the next start).
    pub fn export(&self, gpu: &Gpu) -> io::Result<Vec<(u64, u32)>> {
        let mut cap = self.stats()?[0] as usize;
        loop {
            let dk = DeviceMem::alloc(gpu, 8 * cap.max(1))?;
            let dv = DeviceMem::alloc(gpu, 4 * cap.max(1))?;
            let dc = DeviceMem::alloc(gpu, 4)?;
            let stream = unsafe { sys::sdgpu_stream(*gpu.ctx()) };
            check(unsafe {
                sys::sdgpu_index_export_device(self.0, dk.ptr().cast(), dv.ptr().cast(), cap as u64,
                                               dc.ptr().cast(), stream)
            })?;
            let n = dc.read_u32(gpu)? as usize;
            if n > cap {
                cap = n; // grew since the count was read: once more with room
                continue;
            }
            let mut keys = vec![0u64; n];
            let mut values = vec![0u32; n];
            dk.read_into(gpu, &mut keys)?;
            dv.read_into(gpu, &mut values)?;
            return Ok(keys.into_iter().zip(values).collect());
        }
    }

    /// [live keys, slots in use including removed ones, capacity in slots].
    pub fn stats(&self) -> io::Result<[u64; 3]> {
        let mut out = [0u64; 3];
        check(unsafe { sys::sdgpu_index_stats(self.0, out.as_mut_ptr()) })?;
        Ok(out)
    }
}

/// A device allocation of the context, freed on drop (staging for the index
/// maintenance calls above).
struct DeviceMem<'a> {
    gpu: &'a Gpu,
    p: *mut std::os::raw::c_void,
}

impl<'a> DeviceMem<'a> {
    fn alloc(gpu: &'a Gpu, bytes: usize) -> io::Result<Self> {
        let mut p = ptr::null_mut();
        check(unsafe { sys::sdgpu_alloc_device(*gpu.ctx(), bytes, &mut p) })?;
        Ok(DeviceMem { gpu, p })
    }

    fn from_slice<T: Copy>(gpu: &'a Gpu, src: &[T]) -> io::Result<Self> {
        let bytes = std::mem::size_of_val(src);
        let m = Self::alloc(gpu, bytes.max(1))?;
        let ctx = gpu.ctx();
        let stream = unsafe { sys::sdgpu_stream(*ctx) };
        check(unsafe { sys::sdgpu_memcpy_async(*ctx, m.p, src.as_ptr().cast(), bytes, stream) })?;
        // the source slice may go away before the copy runs
        check(unsafe { sys::sdgpu_sync(*ctx) })?;
        Ok(m)
    }

    fn ptr(&self) -> *mut std::os::raw::c_void {
        self.p
    }

    fn read_into<T: Copy>(&self, gpu: &Gpu, dst: &mut [T]) -> io::Result<()> {
        let ctx = gpu.ctx();
        let stream = unsafe { sys::sdgpu_stream(*ctx) };
        check(unsafe {
            sys::sdgpu_memcpy_async(*ctx, dst.as_mut_ptr().cast(), self.p, std::mem::size_of_val(dst),
                                    stream)
        })?;
        check(unsafe { sys::sdgpu_sync(*ctx) })
    }

    fn read_u32(&self, gpu: &Gpu) -> io::Result<u32> {
        let mut v = [0u32; 1];
        self.read_into(gpu, &mut v)?;
        Ok(v[0])
    }
}

impl Drop for DeviceMem<'_> {
    fn drop(&mut self) {
        // the calls above end with sdgpu_sync: nothing still reads the buffer
        unsafe { sys::sdgpu_free_device(*self.gpu.ctx(), self.p) };
    }
}

/// What one batched read + hash of the candidates gives (FileMetadata::new of
/// every row, mod.rs:107-134): cas bytes, has_key, -errno per row.
pub struct Identified {
    pub cas8: Vec<[u8; 8]>,
    pub has_key: Vec<u8>,
    pub status: Vec<i32>,
}

/// `sizes` None: the library stats every path itself (ABI 6), as the
/// reference's FileMetadata::new does (mod.rs:65,80-81).
pub fn identify(gpu: &Gpu, paths: &[PathBuf], sizes: Option<&[u64]>) -> io::Result<Identified> {
    let n = paths.len();
    if sizes.map_or(false, |s| s.len() != n) {
        return Err(io::Error::new(io::ErrorKind::InvalidInput, "one size per path"));
    }
    let c: Vec<_> = paths.iter().map(|p| cpath(p)).collect();
    let ptrs: Vec<*const c_char> = c.iter().map(|s| s.as_ptr()).collect();
    let mut out = Identified { cas8: vec![[0u8; 8]; n], has_key: vec![0u8; n], status: vec![0i32; n] };
    let ctx = gpu.ctx();
    check(unsafe {
        sys::sdgpu_identify_files(*ctx, ptrs.as_ptr(), sizes.map_or(std::ptr::null(), |s| s.as_ptr()),
                                  n as u32, out.cas8.as_mut_ptr(),
                                  out.has_key.as_mut_ptr(), out.status.as_mut_ptr())
    })?;
    Ok(out)
}

/// `identify` plus the integrity_checksum of every file it read whole, from
/// the same read (`sdgpu_identify_checksum_files`): `has_checksum[i]` is 1 for
/// a row with status 0 whose size is in (0, 100 KiB], and `checksum32[i]` is
/// then BLAKE3 of the bytes that went into its cas_id -- what `file_checksum`
/// (validation/hash.rs:10-24) would have returned at that moment.  The object
/// validator's query (validator_job.rs:100-116: integrity_checksum NULL) then
/// returns only the sampled and the empty files.
pub struct IdentifiedWithChecksums {
    pub rows: Identified,
    pub checksum32: Vec<[u8; 32]>,
    pub has_checksum: Vec<u8>,
}

impl IdentifiedWithChecksums {
    /// The `integrity_checksum` column value of row i (64 hex chars), if any.
    pub fn integrity_checksum(&self, i: usize) -> Option<String> {
        (self.has_checksum[i] != 0).then(|| hex::encode(self.checksum32[i]))
    }
}

pub fn identify_with_checksums(gpu: &Gpu, paths: &[PathBuf], sizes: Option<&[u64]>)
                               -> io::Result<IdentifiedWithChecksums> {
    let n = paths.len();
    if sizes.map_or(false, |s| s.len() != n) {
        return Err(io::Error::new(io::ErrorKind::InvalidInput, "one size per path"));
    }
    let c: Vec<_> = paths.iter().map(|p| cpath(p)).collect();
    let ptrs: Vec<*const c_char> = c.iter().map(|s| s.as_ptr()).collect();
    let mut out = IdentifiedWithChecksums {
        rows: Identified { cas8: vec![[0u8; 8]; n], has_key: vec![0u8; n], status: vec![0i32; n] },
        checksum32: vec![[0u8; 32]; n],
        has_checksum: vec![0u8; n],
    };
    let ctx = gpu.ctx();
    check(unsafe {
        sys::sdgpu_identify_checksum_files(*ctx, ptrs.as_ptr(),
                                           sizes.map_or(std::ptr::null(), |s| s.as_ptr()), n as u32,
                                           out.rows.cas8.as_mut_ptr(), out.rows.has_key.as_mut_ptr(),
                                           out.checksum32.as_mut_ptr(), out.has_checksum.as_mut_ptr(),
                                           out.rows.status.as_mut_ptr())
    })?;
    Ok(out)
}

/// `identify` plus every file's Object kind -- the three outputs of
/// FileMetadata::new (mod.rs:59-97) from one call
/// (`sdgpu_identify_kind_files`): `kind[i]` is the ObjectKind value
/// (crates/file-ext/src/kind.rs) that `Extension::resolve_conflicting(&path,
/// verify_magic)` (magic.rs:176-236) gives on the bytes the call read for the
/// cas_id, for every row with status 0 (empty files included), 0 for failed
/// rows.  `checksums` as in `identify_with_checksums` (None without).
pub struct IdentifiedWithKinds {
    pub rows: Identified,
    pub kind: Vec<i32>,
    pub checksums: Option<(Vec<[u8; 32]>, Vec<u8>)>,
}

pub fn identify_with_kinds(gpu: &Gpu, paths: &[PathBuf], sizes: Option<&[u64]>, verify_magic: bool)
                           -> io::Result<IdentifiedWithKinds> {
    identify_kinds(gpu, paths, sizes, verify_magic, false)
}

/// `with_checksums`: also the integrity_checksum of the files read whole.
pub fn identify_kinds(gpu: &Gpu, paths: &[PathBuf], sizes: Option<&[u64]>, verify_magic: bool,
                      with_checksums: bool) -> io::Result<IdentifiedWithKinds> {
    let n = paths.len();
    if sizes.map_or(false, |s| s.len() != n) {
        return Err(io::Error::new(io::ErrorKind::InvalidInput, "one size per path"));
    }
    let c: Vec<_> = paths.iter().map(|p| cpath(p)).collect();
    let ptrs: Vec<*const c_char> = c.iter().map(|s| s.as_ptr()).collect();
    let mut out = IdentifiedWithKinds {
        rows: Identified { cas8: vec![[0u8; 8]; n], has_key: vec![0u8; n], status: vec![0i32; n] },
        kind: vec![0i32; n],
        checksums: with_checksums.then(|| (vec![[0u8; 32]; n], vec![0u8; n])),
    };
    let (p32, phas) = match out.checksums.as_mut() {
        Some((d, h)) => (d.as_mut_ptr(), h.as_mut_ptr()),
        None => (ptr::null_mut(), ptr::null_mut()),
    };
    let flags = if verify_magic { sys::SDGPU_KIND_VERIFY_MAGIC } else { 0 };
    let ctx = gpu.ctx();
    check(unsafe {
        sys::sdgpu_identify_kind_files(*ctx, ptrs.as_ptr(),
                                       sizes.map_or(std::ptr::null(), |s| s.as_ptr()), n as u32, flags,
                                       out.rows.cas8.as_mut_ptr(), out.rows.has_key.as_mut_ptr(),
                                       p32, phas, out.kind.as_mut_ptr(),
                                       out.rows.status.as_mut_ptr())
    })?;
    Ok(out)
}

/// The grouping of one batch of identified rows against the index (rows in
/// id order, ranks first_rank + i); rows whose read failed take no part.
pub fn group(gpu: &Gpu, idx: &ObjectIndex<'_>, rows: &Identified, first_rank: u32) -> io::Result<Vec<IdentifiedRow>> {
    let n = rows.cas8.len();
    let mut rep = vec![0u32; n];
    let grouped: Vec<u8> =
        rows.has_key.iter().zip(&rows.status).map(|(&h, &s)| (h != 0 && s == 0) as u8).collect();
    let keys: Vec<u64> = rows.cas8.iter().map(|b| u64::from_le_bytes(*b)).collect();
    {
        let ctx = gpu.ctx();
        check(unsafe {
            sys::sdgpu_dedup_batch(*ctx, idx.0, keys.as_ptr(), grouped.as_ptr(), first_rank, n as u32,
                                   sys::SDGPU_IDENTIFIER_CHUNK_SIZE, rep.as_mut_ptr())
        })?;
    }
    Ok((0..n)
        .map(|i| {
            if rows.status[i] != 0 {
                return IdentifiedRow { cas_id: None, link: Link::Failed(check(rows.status[i]).unwrap_err()) };
            }
            let cas_id = (rows.has_key[i] != 0).then(|| hex::encode(rows.cas8[i]));
            let r = first_rank + i as u32;
            let link = if rep[i] == r {
                Link::Create
            } else if rep[i] & sys::SDGPU_REP_EXISTING != 0 {
                Link::Existing(rep[i] & !sys::SDGPU_REP_EXISTING)
            } else {
                Link::Row(rep[i])
            };
            IdentifiedRow { cas_id, link }
        })
        .collect())
}

/// One job step over `paths` (rows in id order; `sizes` from fs::metadata,
/// mod.rs:65) whose first row has rank `first_rank`.
pub fn identify_step(gpu: &Gpu, idx: &ObjectIndex<'_>, paths: &[PathBuf], sizes: Option<&[u64]>,
                     first_rank: u32) -> io::Result<Vec<IdentifiedRow>> {
    let rows = identify(gpu, paths, sizes)?;
    group(gpu, idx, &rows, first_rank)
}
