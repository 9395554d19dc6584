!> Test driver of the growable capacity as a coupled run meets it: a handle created for exactly the bergs the lists hold, the
!! calving source on, and auto_reserve_growth handed to kid_icebergs_init.  Every kid_icebergs_run may calve bergs; without the
!! mode the first of them would stop the run (KID_ECAPACITY through kid_check).  The same population is then run again on a
!! handle whose capacity is given up front and never grows: the two rebuilt lists must be the same bergs, bit for bit.
!!
!! The grid is the stand-alone driver's Cartesian one (driver/icebergs_driver.F90:274-286), the ocean at rest, a uniform
!! calving flux on every cell; &icebergs_nml is read from ./input.nml.
!! Case file (stream): int32 magic 1263093768, gni, gnj, nsteps; real64 gridres, dt, sst, sss, calving_rate, growth;
!! int64 capacity_tight, capacity_roomy, min_free, n; KID_NB_F64 columns of n, KID_NB_I32 columns, ids.
!! Output, for the grown run and then for the roomy one: int64 kid_capacity at the end, int64 rows of the staging arrays, int64
!! m, the rebuilt bergs in traversal order (columns as above).
!! Written and checked by tests/test_reserve_fortran_gpu.py.
program kid_reserve_test
  use, intrinsic :: iso_c_binding
  use kid_hip_mod
  use kid_icebergs_glue
  implicit none
  character(len=1024) :: fin, fout
  integer(c_int32_t) :: magic, gni, gnj, nsteps
  real(c_double) :: gridres, dt, sst0, sss0, calving_rate, growth
  integer(c_int64_t) :: cap_tight, cap_roomy, min_free, n
  integer :: u, uo_, q, i, j
  real(c_double), allocatable :: lon(:,:), lat(:,:), wet(:,:), dx(:,:), dy(:,:), area(:,:), cos_rot(:,:), sin_rot(:,:), depth(:,:)
  real(c_double), allocatable :: f64(:,:)
  integer(c_int32_t), allocatable :: i32(:,:)
  integer(c_int64_t), allocatable :: ids(:)

  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old', action='read')
  read(u) magic
  if (magic /= 1263093768) error stop 'kid_reserve_test: bad magic'
  read(u) gni, gnj, nsteps
  read(u) gridres, dt, sst0, sss0, calving_rate, growth
  read(u) cap_tight, cap_roomy, min_free, n
  allocate(f64(n, KID_NB_F64), i32(n, KID_NB_I32), ids(n))
  do q = 1, KID_NB_F64 ; read(u) f64(:, q) ; enddo
  do q = 1, KID_NB_I32 ; read(u) i32(:, q) ; enddo
  read(u) ids
  close(u)

  allocate(lon(0:gni+1, 0:gnj+1), lat(0:gni+1, 0:gnj+1), wet(0:gni+1, 0:gnj+1), dx(0:gni+1, 0:gnj+1), dy(0:gni+1, 0:gnj+1), &
           area(0:gni+1, 0:gnj+1), cos_rot(0:gni+1, 0:gnj+1), sin_rot(0:gni+1, 0:gnj+1), depth(0:gni+1, 0:gnj+1))
  do j = 0, gnj + 1 ; do i = 0, gni + 1
    lon(i,j) = gridres * real(i, c_double) ; lat(i,j) = gridres * real(j, c_double)
    dx(i,j) = gridres ; dy(i,j) = gridres ; area(i,j) = gridres * gridres
    wet(i,j) = 1. ; cos_rot(i,j) = 1. ; sin_rot(i,j) = 0. ; depth(i,j) = 1000.
  enddo ; enddo

  open(newunit=uo_, file=trim(fout), access='stream', form='unformatted', status='replace', action='write')
  call one_run(cap_tight, .true.)
  call one_run(cap_roomy, .false.)
  close(uo_)

contains

  subroutine one_run(capacity, grow)
    integer(c_int64_t), intent(in) :: capacity
    logical, intent(in) :: grow
    type(kid_glue), target :: bergs
    type(iceberg) :: vals
    type(iceberg), pointer :: this
    integer(c_int64_t) :: k, m, cap_end
    integer :: s, grdi, grdj, c
    real(c_double), allocatable, target :: uo(:,:), vo(:,:), ui(:,:), vi(:,:), tauxa(:,:), tauya(:,:), ssh(:,:), sst(:,:), cn(:,:), hi(:,:), &
        sss(:,:), calving(:,:), calving_hflx(:,:)
    if (grow) then
      call kid_icebergs_init(bergs, gni, gnj, (/1, 1/), (/1, 1/), (/0, 0/), 0, 0, dt, 1, 0._c_double, &
                             lon(1:gni,1:gnj), lat(1:gni,1:gnj), wet, dx, dy, area(1:gni,1:gnj), cos_rot, sin_rot, &
                             ocean_depth=depth(1:gni,1:gnj), fractional_area=.false., capacity=capacity, &
                             auto_reserve_growth=growth, auto_reserve_min_free=min_free)
    else
      call kid_icebergs_init(bergs, gni, gnj, (/1, 1/), (/1, 1/), (/0, 0/), 0, 0, dt, 1, 0._c_double, &
                             lon(1:gni,1:gnj), lat(1:gni,1:gnj), wet, dx, dy, area(1:gni,1:gnj), cos_rot, sin_rot, &
                             ocean_depth=depth(1:gni,1:gnj), fractional_area=.false., capacity=capacity)
    endif
    bergs%f64(1:n, :) = f64 ; bergs%i32(1:n, :) = i32 ; bergs%ids(1:n) = ids
    do k = 1, n
      call row_to_node(bergs, k, vals)
      call kid_glue_add_berg(bergs, vals)
    enddo
    call kid_glue_flatten(bergs)
    allocate(uo(gni+2, gnj+2), vo(gni+2, gnj+2), ui(gni+2, gnj+2), vi(gni+2, gnj+2), tauxa(gni, gnj), tauya(gni, gnj), &
             ssh(gni+2, gnj+2), cn(gni+2, gnj+2), hi(gni+2, gnj+2), sst(gni, gnj), sss(gni, gnj), calving(gni, gnj), calving_hflx(gni, gnj))
    uo = 0. ; vo = 0. ; ui = 0. ; vi = 0. ; tauxa = 0. ; tauya = 0. ; ssh = 0. ; cn = 0. ; hi = 0. ; sst = sst0 ; sss = sss0
    do s = 1, nsteps
      calving = calving_rate ; calving_hflx = 0.
      call kid_icebergs_run(bergs, 1, real(s - 1, c_double) * dt / 86400._c_double, calving, uo, vo, ui, vi, tauxa, tauya, ssh, sst, calving_hflx, cn, hi, sss=sss)
    enddo
    call kid_glue_unflatten(bergs)
    call kid_check(kid_capacity(bergs%h, cap_end), bergs%h, 'kid_capacity')
    m = kid_glue_count(bergs)
    write(uo_) cap_end, bergs%capacity, m
    k = 0
    do grdj = bergs%gd%jsc, bergs%gd%jec ; do grdi = bergs%gd%isc, bergs%gd%iec
      this => bergs%list(grdi,grdj)%first
      do while (associated(this))
        k = k + 1
        call node_to_row(this, bergs, k)
        this => this%next
      enddo
    enddo ; enddo
    do c = 1, KID_NB_F64 ; write(uo_) bergs%f64(1:m, c) ; enddo
    do c = 1, KID_NB_I32 ; write(uo_) bergs%i32(1:m, c) ; enddo
    write(uo_) bergs%ids(1:m)
    write(*,'(a,l1,a,i0,a,i0,a,i0)') 'kid_reserve_test: grow=', grow, ' steps=', nsteps, ' bergs=', m, ' capacity=', cap_end
    call kid_glue_end(bergs)
  end subroutine one_run
end program kid_reserve_test
