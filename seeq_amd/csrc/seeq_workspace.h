/*
 * seeq_workspace.h -- who owns a scan context's buffers: the workspace of seeqdev_scan (seeq_device.hip) as PURE host code.
 *
 * A Workspace knows how memory of three kinds is had and given back (hooks: seeq_device.hip wraps hipMalloc / hipHostMalloc /
 * hipFree / hipHostFree and its copies, tests/host_harness.cpp wraps malloc / memcpy and refuses the N-th request) and which member pointers of its
 * context hold a block (the registry: the address of the pointer and its kind -- a slot enters it the first time it is
 * grown or made).  Three guarantees:
 *
 *   ws_grow   a capacity group grows COMPLETELY OR NOT AT ALL as far as its capacity says: per member, in the listed order, the new
 *             block first, then the old one goes; a refusal returns -1 with the capacity untouched and every slot on a live block
 *             at least as large as that capacity needs (a member may already be on its bigger block).
 *   ws_grow_keep  ONE member that carries its first `keep` bytes over: the new block, the copy (hooks.copy), then the old block goes,
 *             the capacity last; a refusal or a failed copy returns -1 with the new block released and the old one, its contents
 *             and the capacity as they were.
 *   ws_make   fixed-size buffers made on first use, ALL OR NOTHING: a refusal releases what this call made and leaves those slots
 *             NULL -- a "made yet?" guard never sees half a set.
 *
 * and one free path: ws_free_all releases every registered slot -- a buffer that exists is freed by construction.  Nothing is
 * pooled or merged: every member is a block of its own, requested with exactly the size and in exactly the order its site lists.
 * No HIP in here, no heap of its own.
 */
#ifndef SEEQ_WORKSPACE_H_
#define SEEQ_WORKSPACE_H_

#include <stddef.h>
#include <initializer_list>

enum WsKind { WS_DEVICE = 0, WS_PINNED = 1, WS_COHERENT = 2 };      /* device memory; page-locked host memory; the same, fine-grained (coherent) */

struct WsHooks {
   void *(*alloc)(void *ctx, int kind, size_t bytes);      /* NULL: refused (the hook reports why) */
   void  (*release)(void *ctx, int kind, void *p);
   void  *ctx;
   /* ws_grow_keep alone; != 0: failed (the hook reports why).  Last, so a table of alloc / release / ctx (a user of ws_grow and ws_make) needs none */
   int   (*copy)(void *ctx, int kind, void *dst, const void *src, size_t bytes);
};

static constexpr int WS_MAX_SLOTS = 144;

struct Workspace {
   WsHooks hooks;
   struct { void **slot; int kind; } reg[WS_MAX_SLOTS];
   int nreg;
};

/* a member of a group or set: the context's pointer, the bytes it is to hold, its kind */
struct WsMember {
   void **slot; size_t bytes; int kind;
   template <class T> WsMember(T *&p, size_t b, int k = WS_DEVICE) : slot((void **)&p), bytes(b), kind(k) {}
};

/* the registry entry of a slot (entered when new); -1: the registry is full */
static inline int ws_adopt(Workspace *w, void **slot, int kind)
{
   for (int i = 0; i < w->nreg; i++) if (w->reg[i].slot == slot) return i;
   if (w->nreg == WS_MAX_SLOTS) return -1;
   w->reg[w->nreg].slot = slot; w->reg[w->nreg].kind = kind;
   return w->nreg++;
}

static inline int ws_grow(Workspace *w, size_t *cap, size_t want, std::initializer_list<WsMember> members)
{
   if (want <= *cap) return 0;
   for (const WsMember &m : members) {
      if (ws_adopt(w, m.slot, m.kind) < 0) return -1;
      void *g = w->hooks.alloc(w->hooks.ctx, m.kind, m.bytes);
      if (!g) return -1;
      if (*m.slot) w->hooks.release(w->hooks.ctx, m.kind, *m.slot);
      *m.slot = g;
   }
   *cap = want;
   return 0;
}

static inline int ws_grow_keep(Workspace *w, size_t *cap, size_t want, WsMember m, size_t keep)
{
   if (want <= *cap) return 0;
   if (ws_adopt(w, m.slot, m.kind) < 0) return -1;
   void *g = w->hooks.alloc(w->hooks.ctx, m.kind, m.bytes);
   if (!g) return -1;
   if (*m.slot && keep && w->hooks.copy(w->hooks.ctx, m.kind, g, *m.slot, keep)) { w->hooks.release(w->hooks.ctx, m.kind, g); return -1; }
   if (*m.slot) w->hooks.release(w->hooks.ctx, m.kind, *m.slot);
   *m.slot = g;
   *cap = want;
   return 0;
}

/* every member whose slot is NULL is made; 0: all of them hold a block now */
static inline int ws_make(Workspace *w, std::initializer_list<WsMember> members)
{
   const WsMember *made[16];
   int nmade = 0;
   for (const WsMember &m : members) {
      if (*m.slot) continue;
      void *g = nmade < 16 && ws_adopt(w, m.slot, m.kind) >= 0 ? w->hooks.alloc(w->hooks.ctx, m.kind, m.bytes) : NULL;
      if (!g) {
         while (nmade--) { w->hooks.release(w->hooks.ctx, made[nmade]->kind, *made[nmade]->slot); *made[nmade]->slot = NULL; }
         return -1;
      }
      *m.slot = g;
      made[nmade++] = &m;
   }
   return 0;
}

static inline void ws_release_at(Workspace *w, int i)
{
   if (!*w->reg[i].slot) return;
   w->hooks.release(w->hooks.ctx, w->reg[i].kind, *w->reg[i].slot);
   *w->reg[i].slot = NULL;
}

/* one buffer given back ahead of the rest (its slot stays registered) */
template <class T> static inline void ws_release(Workspace *w, T *&p)
{
   for (int i = 0; i < w->nreg; i++) if (w->reg[i].slot == (void **)&p) ws_release_at(w, i);
}

static inline void ws_free_all(Workspace *w)
{
   for (int i = 0; i < w->nreg; i++) ws_release_at(w, i);
   w->nreg = 0;
}

#endif
