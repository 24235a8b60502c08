//! Sync ingest (core/crates/sync/src/ingest.rs:114-233): which CRDT operations
//! of a received page apply, decided for the whole page by one call
//! (`sdgpu_sync_ingest`) against a device-resident op log.
//!
//! An op is old exactly when the log holds an op of its (model, record_id,
//! kind) -- or (relation, item_id, kind) -- with a larger timestamp in SIGNED
//! int64 order (`compare_message`, ingest.rs:188-233); an op that is not old is
//! applied and logged (ingest.rs:162-186), so later ops of the page see it.  The
//! instance clocks take the UNSIGNED NTP64 order (ingest.rs:119-126,151).
//! `get_ops` (manager.rs:130-199), the writes of `apply_op`, the HLC and the
//! transport stay with the caller.
//!
//! Keys and tags are two independent 64-bit hashes of the tuple; a non-zero
//! `collisions` means two tuples share a key: re-key with another salt and
//! reload the log.  The case is detected, not repaired.

use std::{io, ptr};

use sdgpu_sys as sys;

use crate::{check, Gpu};

/// One page, or the rows of the op log, as columns.  `timestamps` are the
/// NTP64 values `as_u64() as i64`.
pub struct Ops<'a> {
    pub keys: &'a [u64],
    pub tags: &'a [u64],
    pub timestamps: &'a [i64],
    /// Index of each op's instance into the clocks, with the clocks.
    pub instances: Option<(&'a [u32], &'a mut [u64])>,
}

pub struct Decision {
    pub apply: Vec<u8>,
    /// Ops to apply and log, ascending (page order).
    pub applied: Vec<u32>,
    /// The highest applied op of every key: the value that survives in the row.
    pub winners: Vec<u32>,
    pub new_keys: u32,
    pub collisions: u32,
}

/// key -> newest logged timestamp; lives as long as the library is open.
pub struct OpLog<'g> {
    gpu: &'g Gpu,
    raw: *mut sys::sdgpu_oplog,
}

unsafe impl Send for OpLog<'_> {}

impl<'g> OpLog<'g> {
    pub fn new(gpu: &'g Gpu, capacity_hint: u64) -> io::Result<Self> {
        let mut raw = ptr::null_mut();
        let ctx = gpu.ctx();
        check(unsafe { sys::sdgpu_oplog_create(*ctx, capacity_hint, &mut raw) })?;
        drop(ctx);
        Ok(OpLog { gpu, raw })
    }

    /// (keys stored, capacity in slots).
    pub fn stats(&self) -> io::Result<(u64, u64)> {
        let mut out = [0u64; 2];
        let _ctx = self.gpu.ctx();
        check(unsafe { sys::sdgpu_oplog_stats(self.raw, out.as_mut_ptr()) })?;
        Ok((out[0], out[1]))
    }

    /// Loads existing op-log rows, in any order: afterwards the log holds the
    /// maximum of every key (a page whose decisions are dropped).  The ABI has no
    /// host-array form of `sdgpu_oplog_add_device`, so this costs a full ingest
    /// of the rows (three outputs of their length, the sort and the scan); a
    /// caller with the rows on the device uses `sdgpu_oplog_add_device`.
    pub fn load(&self, rows: Ops<'_>) -> io::Result<u32> {
        Ok(self.ingest(rows, true)?.collisions)
    }

    /// Decides one page in arrival order.  `commit == false`
    /// (`SDGPU_INGEST_NO_COMMIT`): no timestamp in the log changes; the caller
    /// commits the ops it managed to apply with `load`.
    pub fn ingest(&self, ops: Ops<'_>, commit: bool) -> io::Result<Decision> {
        let n = ops.keys.len();
        if ops.tags.len() != n
            || ops.timestamps.len() != n
            || ops.instances.as_ref().map_or(false, |(i, _)| i.len() != n)
        {
            return Err(io::Error::from_raw_os_error(libc::EINVAL));
        }
        let mut out = Decision {
            apply: vec![0u8; n],
            applied: vec![0u32; n],
            winners: vec![0u32; n],
            new_keys: 0,
            collisions: 0,
        };
        let mut counts = [0u32; 4];
        let (inst, clock, n_inst) = match ops.instances {
            Some((i, c)) => (i.as_ptr(), c.as_mut_ptr(), c.len() as u32),
            None => (ptr::null(), ptr::null_mut(), 0),
        };
        let flags = if commit { 0 } else { sys::SDGPU_INGEST_NO_COMMIT };
        let _ctx = self.gpu.ctx();
        check(unsafe {
            sys::sdgpu_sync_ingest(self.raw, ops.keys.as_ptr(), ops.tags.as_ptr(),
                                   ops.timestamps.as_ptr(), inst, n as u64, clock, n_inst, flags,
                                   out.apply.as_mut_ptr(), out.applied.as_mut_ptr(),
                                   out.winners.as_mut_ptr(), counts.as_mut_ptr())
        })?;
        out.applied.truncate(counts[0] as usize);
        out.winners.truncate(counts[1] as usize);
        out.new_keys = counts[2];
        out.collisions = counts[3];
        Ok(out)
    }
}

impl Drop for OpLog<'_> {
    fn drop(&mut self) {
        let _ctx = self.gpu.ctx();
        unsafe { sys::sdgpu_oplog_destroy(self.raw) };
    }
}
