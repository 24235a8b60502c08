//! The explorer's search page (core/src/api/search.rs:393-562, `search.paths`;
//! :563-582, `pathsCount`): the WHERE clause over file_path and its Object,
//! `ORDER BY is_dir DESC, <field>, id`, the keyset cursor or the offset and the
//! `take`, answered by one call (`sdgpu_search_page`) over columns the caller
//! holds in memory.  The semantics -- SQLite's three-valued logic, the cursor
//! arms of :463-475 with their descending `id <`, NULL keys lowest -- are
//! stated in include/sdgpu.h.
//!
//! Deviation: where the reference gives no final id order (OrderOnly, Offset)
//! ties go by ascending id, one of the orders SQLite may return.

use std::{io, ptr};

use sdgpu_sys as sys;

use crate::{check, Gpu};

/// One table's file_path rows in ascending id order; a column the query does
/// not use may be `None`.
#[derive(Default)]
pub struct Rows<'a> {
    pub n: usize,
    pub location: Option<&'a [i32]>,
    pub ext: Option<&'a [u16]>,
    pub dir_key: Option<&'a [u64]>,
    pub flags: Option<&'a [u8]>,
    pub date_created: Option<&'a [i64]>,
    pub object: Option<&'a [i32]>,
    pub eligible: Option<&'a [u8]>,
    pub order_key: Option<&'a [i64]>,
}

/// The Object columns `Rows::object` indexes, and the tag_on_object pairs.
#[derive(Default)]
pub struct Objects<'a> {
    pub m: usize,
    pub kind: Option<&'a [i32]>,
    pub flags: Option<&'a [u8]>,
    pub date_accessed: Option<&'a [i64]>,
    pub order_key: Option<&'a [i64]>,
    pub tag_obj: &'a [i32],
    pub tag_tag: &'a [i32],
}

pub struct Page {
    /// Row indices of the candidates of ranks `[offset, offset + take)`.
    pub rows: Vec<u32>,
    /// Matching rows (pathsCount), candidates, rows.len(), directories among
    /// the matching rows.
    pub counts: [u32; 4],
}

fn col<T>(c: Option<&[T]>, n: usize) -> io::Result<*const T> {
    match c {
        Some(s) if s.len() != n => Err(io::Error::from_raw_os_error(libc::EINVAL)),
        Some(s) => Ok(s.as_ptr()),
        None => Ok(ptr::null()),
    }
}

fn structs(rows: &Rows<'_>, objects: Option<&Objects<'_>>)
           -> io::Result<(sys::sdgpu_search_rows_t, Option<sys::sdgpu_search_objects_t>)> {
    let n = rows.n;
    let r = sys::sdgpu_search_rows_t {
        n: n as u64,
        location: col(rows.location, n)?,
        ext: col(rows.ext, n)?,
        dir_key: col(rows.dir_key, n)?,
        flags: col(rows.flags, n)?,
        date_created: col(rows.date_created, n)?,
        object: col(rows.object, n)?,
        eligible: col(rows.eligible, n)?,
        order_key: col(rows.order_key, n)?,
    };
    let o = match objects {
        None => None,
        Some(o) => {
            if o.tag_obj.len() != o.tag_tag.len() {
                return Err(io::Error::from_raw_os_error(libc::EINVAL));
            }
            Some(sys::sdgpu_search_objects_t {
                m: o.m as u64,
                kind: col(o.kind, o.m)?,
                flags: col(o.flags, o.m)?,
                date_accessed: col(o.date_accessed, o.m)?,
                order_key: col(o.order_key, o.m)?,
                tag_obj: o.tag_obj.as_ptr(),
                tag_tag: o.tag_tag.as_ptr(),
                n_pairs: o.tag_obj.len() as u64,
            })
        }
    };
    Ok((r, o))
}

/// One page: `query.take` rows at the most (`SDGPU_SEARCH_MAX_TAKE`).
pub fn search_page(gpu: &Gpu, rows: &Rows<'_>, objects: Option<&Objects<'_>>,
                   query: &sys::sdgpu_search_query_t) -> io::Result<Page> {
    let (r, o) = structs(rows, objects)?;
    let mut page = vec![0u32; sys::SDGPU_SEARCH_MAX_TAKE as usize];
    let mut counts = [0u32; 4];
    let ctx = gpu.ctx();
    check(unsafe {
        sys::sdgpu_search_page(*ctx, &r, o.as_ref().map_or(ptr::null(), |o| o as *const _), query,
                               page.as_mut_ptr(), counts.as_mut_ptr())
    })?;
    page.truncate(counts[2] as usize);
    Ok(Page { rows: page, counts })
}

/// `pathsCount`: the rows the filter of `query` matches (take and the
/// pagination are ignored).
pub fn paths_count(gpu: &Gpu, rows: &Rows<'_>, objects: Option<&Objects<'_>>,
                   query: &sys::sdgpu_search_query_t) -> io::Result<u32> {
    let mut q = *query;
    q.take = 0;
    q.offset = 0;
    q.flags &= !(sys::SDGPU_SEARCH_CURSOR | sys::SDGPU_SEARCH_CURSOR_STRICT);
    let (r, o) = structs(rows, objects)?;
    let mut counts = [0u32; 4];
    let ctx = gpu.ctx();
    check(unsafe {
        sys::sdgpu_search_page(*ctx, &r, o.as_ref().map_or(ptr::null(), |o| o as *const _), &q,
                               ptr::null_mut(), counts.as_mut_ptr())
    })?;
    Ok(counts[0])
}
