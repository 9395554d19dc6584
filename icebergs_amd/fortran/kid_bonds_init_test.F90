!> Test driver of the bonded tail of icebergs_init (IB:153-171) with manually_initialize_bonds: the namelist group icebergs_nml
!! read from ./input.nml, bergs as heap nodes in per-cell lists WITHOUT bonds, kid_icebergs_init_bonds forms the bonds on the
!! device (kid_initialize_bonds), rebuilds the `bond` lists and does the rest of the tail (n_bonds, dem_tests_init).
!!
!! The stand-alone driver's Cartesian grid as in kid_init_test.F90 (driver/icebergs_driver.F90:274-286).
!! Case file (stream): int32 magic 1263093766, gni, gnj, dom_x_flags; real64 gridres, dt; int64 capacity, n;
!! KID_NB_F64 columns of n, KID_NB_I32 columns, ids (file order: insert_berg_into_list sorts).
!! Output: int64 m; per berg in traversal order: int64 id, int32 n_bonds, int32 count, then per bond in list order int64
!! other_id, int64 id of other_berg (-1 when not connected), int32 broken, int32 pad.
!! Written and checked by tests/test_fortran_bond_init_gpu.py.
program kid_bonds_init_test
  use, intrinsic :: iso_c_binding
  use kid_hip_mod
  use kid_icebergs_glue
  implicit none
  character(len=1024) :: fin, fout
  type(kid_glue), target :: bergs
  type(iceberg) :: vals
  type(iceberg), pointer :: this
  type(bond), pointer :: b
  integer(c_int32_t) :: magic, gni, gnj, dom_x_flags, cnt
  real(c_double) :: gridres, dt
  integer(c_int64_t) :: capacity, n, k, m, oid
  integer :: u, uo_, q, i, j, grdi, grdj
  real(c_double), allocatable :: lon(:,:), lat(:,:), wet(:,:), dx(:,:), dy(:,:), area(:,:), cos_rot(:,:), sin_rot(:,:), depth(:,:)

  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old', action='read')
  read(u) magic
  if (magic /= 1263093766) error stop 'kid_bonds_init_test: bad magic'
  read(u) gni, gnj, dom_x_flags
  read(u) gridres, dt
  read(u) capacity, n

  allocate(lon(0:gni+1, 0:gnj+1), lat(0:gni+1, 0:gnj+1), wet(0:gni+1, 0:gnj+1), dx(0:gni+1, 0:gnj+1), dy(0:gni+1, 0:gnj+1), &
           area(0:gni+1, 0:gnj+1), cos_rot(0:gni+1, 0:gnj+1), sin_rot(0:gni+1, 0:gnj+1), depth(0:gni+1, 0:gnj+1))
  do j = 0, gnj + 1 ; do i = 0, gni + 1
    lon(i,j) = gridres * real(i, c_double) ; lat(i,j) = gridres * real(j, c_double)
    dx(i,j) = gridres ; dy(i,j) = gridres ; area(i,j) = gridres * gridres
    wet(i,j) = 1. ; cos_rot(i,j) = 1. ; sin_rot(i,j) = 0. ; depth(i,j) = 1000.
  enddo ; enddo

  call kid_icebergs_init(bergs, gni, gnj, (/1, 1/), (/1, 1/), (/0, 0/), dom_x_flags, 0, dt, 1, 0._c_double, &
                         lon(1:gni,1:gnj), lat(1:gni,1:gnj), wet, dx, dy, area(1:gni,1:gnj), cos_rot, sin_rot, &
                         ocean_depth=depth(1:gni,1:gnj), fractional_area=.false., capacity=capacity)

  do q = 1, KID_NB_F64 ; read(u) bergs%f64(1:n, q) ; enddo
  do q = 1, KID_NB_I32 ; read(u) bergs%i32(1:n, q) ; enddo
  read(u) bergs%ids(1:n)
  close(u)
  do k = 1, n
    call row_to_node(bergs, k, vals)
    call kid_glue_add_berg(bergs, vals)
  enddo
  call kid_icebergs_init_bonds(bergs)

  open(newunit=uo_, file=trim(fout), access='stream', form='unformatted', status='replace', action='write')
  m = kid_glue_count(bergs)
  write(uo_) m
  do grdj = bergs%gd%jsc, bergs%gd%jec ; do grdi = bergs%gd%isc, bergs%gd%iec
    this => bergs%list(grdi,grdj)%first
    do while (associated(this))
      cnt = 0
      b => this%first_bond
      do while (associated(b)) ; cnt = cnt + 1 ; b => b%next_bond ; enddo
      write(uo_) this%id, int(this%n_bonds, c_int32_t), cnt
      b => this%first_bond
      do while (associated(b))
        oid = -1 ; if (associated(b%other_berg)) oid = b%other_berg%id
        write(uo_) b%other_id, oid, int(b%broken, c_int32_t), 0_c_int32_t
        b => b%next_bond
      enddo
      this => this%next
    enddo
  enddo ; enddo
  close(uo_)
  write(*,'(a,i0)') 'kid_bonds_init_test: bergs=', m
  call kid_glue_end(bergs)
end program kid_bonds_init_test
